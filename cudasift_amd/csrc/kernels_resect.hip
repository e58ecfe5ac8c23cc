// kernels_resect.hip — misift_resect_cameras_batch: the camera of each selected image estimated directly from the
// observations its image makes of the triangulated track points, by batch RANSAC over calibrated six-point solves.  It
// places the images that the walk of misift_link_poses_batch never reached, and gives a placed image a second opinion that
// does not rest on the chain of pair poses.  No reference counterpart.  The arithmetic is resect_core.hpp (the draw, the
// solve) and refine_core.hpp (the inlier test), shared with the host-only test hooks at the end of this file.
//
// The search is ransac_batch.hpp's with ResectModel (resect_model.hpp: the model, the solve of a lane and the entry's
// results, shared with misift_localize_frames_batch).  What is this file's: two memsets (the owners, the summary)
// and, whatever the data, six launches (nsel == 0: the summary's memset and the pick launch alone, which writes T):
//   cand_owner_kernel     the owner of every slot and
//   cand_key_kernel       the image every slot is a candidate of: launch_track_candidates (track_candidates.hpp), in the
//                         gather's scope; owner and key are the prefix of the search's temp.
//   resect_gather_kernel  walks the keys in ascending slot order; the lane of a candidate writes its x, y, X, Y, Z.
//                         Entries that are skipped (only_unset), hold more than max_cand candidates (counted, not stored)
//                         or fewer than max(6, min_inliers) are marked done here.
//   resect_solve_kernel   each lane's 11 x 12 system lives in LDS, word (r, c) of lane l at (12 r + c) * 64 + l, so every
//                         access of the wavefront hits 64 consecutive words whatever rows and columns the lanes have
//                         pivoted to: 33 KiB per workgroup.
//   (count)               ransac_count_kernel<ResectModel>: refine_member under the image's intrinsics, 10 KiB of LDS.
//   resect_pick_kernel    the entry's results, the install, the summary.
// Not built: a minimal P3P solver, a local optimisation inside the search, a 32-hypothesis solve workgroup.
#include <stdint.h>
#include <string.h>
#include "common.hpp"
#include "ransac_batch.hpp"
#include "resect_core.hpp"
#include "resect_model.hpp"
#include "track_candidates.hpp"

namespace {

struct ResectArgs {
  RansacSearch rs;                             // coord: x, y, X, Y, Z of the candidates in slot order; meta[1] a done
                                               // entry's status, [2] what d_res_cand gets
  TrackScene s;                                // intrinsics: the pinned host copy; cam and cam_pair may be NULL
  const int *owner, *key;                      // temp ahead of the search's: max_obs each
  int max_cand;
  int min_inliers, only_unset, install;
  const int *images;                           // the pinned host copy: nsel
  float *cam;                                  // in/out: nimages x 12, written under install
  int *cam_pair;                               // in/out: nimages
  float *res_cam;
  int *res_cand, *res_inliers, *res_status, *summary;
};

typedef ResectModelOf<ResectArgs, false> ResectModel;     // resect_model.hpp, shared with the localise search

__global__ __launch_bounds__(1024) void resect_gather_kernel(ResectArgs A)
{
  const RansacSearch &S = A.rs;
  const int e = blockIdx.x, tid = threadIdx.x;
  const int img = A.images[e];                 // checked on the host: in [0, nimages)
  int *meta = S.meta + (size_t)RANSAC_META * e;
  if (A.only_unset && A.cam_pair[img] != POSEGRAPH_UNSET) {
    if (tid == 0) { meta[0] = 0; meta[1] = RESECT_SKIPPED; meta[2] = 0; }
    return;
  }
  const int O = scene_O(A.s), T = scene_T(A.s);
  const int mc = S.cap16;
  float *coord = S.coord + (size_t)e * 5 * mc;
  const RansacCompaction c = ransac_compaction();
  for (long long o0 = 0; o0 < O; o0 += 1024) {
    const long long o = o0 + tid;
    const bool ok = o < O && A.key[o] == img;
    const int pos = c.place(ok);
    if (ok && pos < A.max_cand) {              // beyond max_cand only the count goes on
      const int t = A.owner[o];
      const bool t_ok = (unsigned)t < (unsigned)T;           // an index from device memory: checked before use
      const float *P = A.s.points + 4 * (size_t)(t_ok ? t : 0);
      const TrackObs ob = track_obs_load(A.s.obs + o);
      coord[pos] = ob.xpos;
      coord[mc + pos] = ob.ypos;
      coord[2 * mc + pos] = t_ok ? P[0] : 0.0f;
      coord[3 * mc + pos] = t_ok ? P[1] : 0.0f;
      coord[4 * mc + pos] = t_ok ? P[2] : 0.0f;
    }
    c.next();
  }
  const int n = c.total();
  const int need = A.min_inliers > RESECT_SAMPLE ? A.min_inliers : RESECT_SAMPLE;
  if (n > A.max_cand || n < need) {
    if (tid == 0) { meta[0] = 0; meta[1] = n > A.max_cand ? RESECT_OVER : RESECT_FEW_CAND; meta[2] = n; }
    return;
  }
  if (tid < 64) {                              // wave 0
    ransac_draw<ResectModel>(S.seeds[e], n, S.sample + (size_t)e * RESECT_SAMPLE * S.lp, S.num_loops, S.lp);
    if (tid == 0) { meta[0] = n; meta[1] = 0; meta[2] = n; }
  }
}

__global__ __launch_bounds__(64) void resect_solve_kernel(ResectArgs A, int hblocks)
{
  __shared__ float s_m[RESECT_SOLVE_LDS];
  resect_solve_lane<ResectModel>(A, hblocks, s_m);
}

__global__ __launch_bounds__(1024) void resect_pick_kernel(ResectArgs A)
{
  const RansacSearch &S = A.rs;
  const int e = blockIdx.x, tid = threadIdx.x;
  if (e == 0 && tid == 0) A.summary[0] = scene_T(A.s);
  if (e >= S.nsel) return;                     // nsel == 0: the one workgroup that writes T
  const int *meta = S.meta + (size_t)RANSAC_META * e;
  const bool searched = meta[0] != 0;
  unsigned long long best = 0;
  if (searched) best = ransac_pick(S.hcount + (size_t)e * S.lp, S.num_loops);
  if (tid != 0) return;
  int picked;
  resect_entry_results(A, e, searched, best, &picked);
}

// the candidates an entry's temp has room for: an image has no more than O <= max_obs, so n > max_cand decides as stated
int resect_capacity(int max_obs, int max_cand) { return min(max_cand, min(max_obs, 0x7fffffff - 15)); }

}  // namespace

bool resect_cameras_batch_one_launch(int max_obs, int nsel, int max_cand, int num_loops)
{
  return ransac_one_launch(nsel, resect_capacity(max_obs, max_cand), num_loops);
}

// Enqueue misift_resect_cameras_batch on the context stream (common.hpp): two memsets and six launches.
int launch_resect_cameras_batch(misift_ctx *ctx, const TrackScene &scene, int nsel, const int *h_images,
                                const unsigned *h_seeds, int max_cand, int num_loops, float thresh2, int min_inliers,
                                int only_unset, int install, float *d_cam, int *d_cam_pair, float *d_res_cam,
                                int *d_res_cand, int *d_res_inliers, int *d_res_status, int *d_summary)
{
  const RansacNames names{"misift_resect_cameras_batch", "candidates", "resect_gather", "resect_solve", "resect_count",
                          "resect_pick"};
  const int max_obs = scene.max_obs;
  ResectArgs A{};
  int rc = ransac_search(names, nsel, resect_capacity(max_obs, max_cand), num_loops, thresh2, h_seeds, A.rs);
  if (!rc) rc = ransac_temp<ResectModel>(ctx, A.rs, 2 * sizeof(int) * (size_t)max_obs, 0, nullptr);
  if (rc) return rc;
  int *owner = reinterpret_cast<int *>(ctx->d_match_tmp), *key = owner + max_obs;
  A.s = scene;
  A.owner = owner; A.key = key;
  A.max_cand = max_cand;
  A.min_inliers = min_inliers; A.only_unset = only_unset; A.install = install;
  A.images = h_images;
  A.cam = d_cam; A.cam_pair = d_cam_pair;
  A.res_cam = d_res_cam; A.res_cand = d_res_cand; A.res_inliers = d_res_inliers; A.res_status = d_res_status;
  A.summary = d_summary;
  HIP_TRY(hipMemsetAsync(d_summary, 0, 8 * sizeof(int), ctx->stream));
  const auto pick = [&] { hipLaunchKernelGGL(resect_pick_kernel, dim3(max(nsel, 1)), dim3(1024), 0, ctx->stream, A); };
  if (nsel == 0) return ransac_scope(ctx, names.pick, pick);
  HIP_TRY(hipMemsetAsync(owner, 0xff, sizeof(int) * (size_t)max_obs, ctx->stream));
  return ransac_launches<ResectModel>(
      ctx, names, A,
      [&] {
        launch_track_candidates(ctx, scene, owner, key);
        hipLaunchKernelGGL(resect_gather_kernel, dim3(nsel), dim3(1024), 0, ctx->stream, A);
      },
      resect_solve_kernel, pick);
}

// Test-only, host-only: the sample draw and the six-point solve as the kernels compute them (resect_core.hpp).
extern "C" int misift_test_resect_samples(unsigned seed, int n, int num_loops, int *out)
{
  if (n < RESECT_SAMPLE || num_loops < 0 || (num_loops > 0 && !out)) {
    misift_set_error("misift_test_resect_samples: invalid argument");
    return MISIFT_EINVAL;
  }
  ransac_host_samples(seed, n, num_loops, out, resect_draw6<LibcRandArrayRing>);
  return MISIFT_OK;
}

extern "C" int misift_test_resect_solve(const float *xyXYZ, const float *intrinsics4, float *cam12, int *valid)
{
  if (!xyXYZ || !intrinsics4 || !cam12 || !valid) {
    misift_set_error("misift_test_resect_solve: invalid argument");
    return MISIFT_EINVAL;
  }
  float x[6], y[6], X[6], Y[6], Z[6], cam[12];
  for (int k = 0; k < 6; k++) {
    x[k] = xyXYZ[5 * k]; y[k] = xyXYZ[5 * k + 1];
    X[k] = xyXYZ[5 * k + 2]; Y[k] = xyXYZ[5 * k + 3]; Z[k] = xyXYZ[5 * k + 4];
  }
  ResectArrayMat m;
  *valid = resect_solve6(m, x, y, X, Y, Z, intrinsics4, cam) ? 1 : 0;
  for (int k = 0; k < 12; k++) cam12[k] = cam[k];
  return MISIFT_OK;
}
