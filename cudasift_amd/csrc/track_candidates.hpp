// track_candidates.hpp — which observation slot is a candidate of which image: the two launches that
// misift_refine_cameras_batch, misift_resect_cameras_batch and misift_adjust_bundle_batch start with, and the first of
// them alone for misift_filter_tracks_batch.  The rule (T, O, valid tracks, the owner of a slot, the candidates of an
// image) is stated once, in include/misift.h under misift_refine_cameras_batch, and written once, in
// triangulate_core.hpp (scene_track_owns, scene_slot_key).  The kernels are compiled once, in
// kernels_track_candidates.hip; the files that include this call launch_track_candidates.
#pragma once
#include "common.hpp"
#include "triangulate_core.hpp"

// Enqueue on ctx->stream, inside the caller's LaunchScope and after the caller's memset of owner[0 .. max_obs) to -1:
//   cand_owner_kernel  256-thread workgroups, one lane per track, the grid sized from max_tracks.  T and O are read from
//                      the export summary on the device.  A lane whose track is valid walks its range with
//                      atomicMax(owner[o], t), so a slot ends with the largest valid track that holds it.
//   cand_key_kernel    one lane per slot, the grid sized from max_obs: key[o] = the observation's frame when slot o is a
//                      candidate of that image, otherwise -1.  Not launched when key is NULL (the owners only).
void launch_track_candidates(misift_ctx *ctx, const TrackScene &scene, int *owner, int *key);
