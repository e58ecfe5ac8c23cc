// kernels_pose.hip — misift_recover_pose_batch: the relative camera pose of every selected frame pair from its
// fundamental matrix and its intrinsics, and the two-view depth of every record.  Entry e works on frame frames[e] of a
// device-resident record batch (counts and offsets read on the device) and writes result slot e; no host round trip.  No
// reference counterpart.  The arithmetic is pose_core.hpp, shared with the host-only test hooks at the end of this file.
//
// One launch, one 256-thread workgroup per entry, the shape of fund_batch_score_kernel:
//   decompose  thread 0 runs steps 1-4 (E, six Jacobi sweeps, the bases, the hypotheses): a serial chain of 18 rotations
//              that no other lane can shorten.  The two rotations and t, 21 floats, go to the others through LDS.
//   vote       each thread walks its records r = t, t + 256, ...: the gate and the inlier test under F, then the depth
//              terms under Ra and Rb from registers; -t flips the sign of n1 and n2 and nothing else, so the four votes
//              cost two evaluations.  Integer sums: a wave reduction, then one LDS atomic per wave and hypothesis.
//   write      the winner's pose, its vote and the four votes; with d_xyz, a second walk over every record of the frame
//              under the winner.  The records are read again from global memory, all within their first 64 bytes: the
//              frame of a pair is a few hundred KiB at the most and the second walk finds it in the L2.
#include <math.h>
#include "common.hpp"
#include "pose_core.hpp"

namespace {

constexpr int POSE_THREADS = 256;

struct FbPoseArgs {
  BatchLayout set;
  const int *frames;                           // pinned host copies of the caller's lists
  const float *K;                              // nsel x 8
  float min_score, max_ambiguity, thresh2;
  const float *F;                              // nsel x 9
  float *pose;                                 // out: nsel x 12
  int *num_front;                              // out: nsel
  int *votes;                                  // out: nsel x 4, may be NULL
  float *xyz;                                  // out: 4 floats per record of the batch, may be NULL
};

__global__ __launch_bounds__(POSE_THREADS) void fund_batch_pose_kernel(FbPoseArgs B)
{
  __shared__ float s_h[21];
  __shared__ int s_valid, s_votes[4];
  const int e = blockIdx.x, f = B.frames[e];
  const int n = max(B.set.counts[f], 0);
  const long long base = B.set.base(f);
  const SiftPointD *pts = B.set.recs + base;
  float F[9];
#pragma unroll
  for (int k = 0; k < 9; k++) F[k] = B.F[(size_t)9 * e + k];
  const float *k8 = B.K + (size_t)8 * e;
  const PoseIntrinsics K{k8[0], k8[1], k8[2], k8[3], k8[4], k8[5], k8[6], k8[7]};
  PoseHypotheses h;
  if (threadIdx.x == 0) {
    s_valid = pose_decompose(F, K, h) ? 1 : 0;
#pragma unroll
    for (int j = 0; j < 9; j++) { s_h[j] = h.Ra[j]; s_h[9 + j] = h.Rb[j]; }
#pragma unroll
    for (int j = 0; j < 3; j++) s_h[18 + j] = h.t[j];
  }
  if (threadIdx.x < 4) s_votes[threadIdx.x] = 0;
  __syncthreads();
  const bool valid = s_valid != 0;
#pragma unroll
  for (int j = 0; j < 9; j++) { h.Ra[j] = s_h[j]; h.Rb[j] = s_h[9 + j]; }
#pragma unroll
  for (int j = 0; j < 3; j++) h.t[j] = s_h[18 + j];

  int v[4] = {0, 0, 0, 0};
  if (valid) {
    for (int i = threadIdx.x; i < n; i += POSE_THREADS) {
      const SiftPointD &pt = pts[i];
      const float x1 = pt.xpos, y1 = pt.ypos, x2 = pt.match_xpos, y2 = pt.match_ypos;
      float sden;
      const float e2 = fundamental_sampson(F, x1, y1, x2, y2, sden);
      const bool gate = pt.score > B.min_score && pt.ambiguity < B.max_ambiguity;
      if (!(gate && fundamental_inlier(e2, sden, B.thresh2))) continue;
      float p1[3], p2[3], den, n1, n2;
      pose_normalised(K, x1, y1, x2, y2, p1, p2);
      pose_depth_terms(h.Ra, h.t, p1, p2, den, n1, n2);
      v[0] += pose_in_front(den, n1, n2) ? 1 : 0;
      v[1] += pose_in_front(den, -n1, -n2) ? 1 : 0;
      pose_depth_terms(h.Rb, h.t, p1, p2, den, n1, n2);
      v[2] += pose_in_front(den, n1, n2) ? 1 : 0;
      v[3] += pose_in_front(den, -n1, -n2) ? 1 : 0;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
    if ((threadIdx.x & 63) == 0 && v[k]) atomicAdd(&s_votes[k], v[k]);
  }
  __syncthreads();
  int best = 0;                                // the largest vote at the smallest k
#pragma unroll
  for (int k = 1; k < 4; k++) best = s_votes[k] > s_votes[best] ? k : best;
  float pose[12];
  pose_hypothesis(h, best, pose);              // zeros for an invalid entry
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < 12; j++) B.pose[(size_t)12 * e + j] = pose[j];
    B.num_front[e] = s_votes[best];
  }
  if (B.votes && threadIdx.x < 4) B.votes[(size_t)4 * e + threadIdx.x] = s_votes[threadIdx.x];
  if (!B.xyz) return;
  float R[9], t[3];
#pragma unroll
  for (int j = 0; j < 9; j++) R[j] = pose[j];
#pragma unroll
  for (int j = 0; j < 3; j++) t[j] = pose[9 + j];
  float *xyz = B.xyz + (size_t)base * 4;
  for (int i = threadIdx.x; i < n; i += POSE_THREADS) {
    const SiftPointD &pt = pts[i];
    float p1[3], p2[3], den, n1, n2, out[4];
    pose_normalised(K, pt.xpos, pt.ypos, pt.match_xpos, pt.match_ypos, p1, p2);
    pose_depth_terms(R, t, p1, p2, den, n1, n2);
    pose_xyz(valid, den, n1, n2, p1, out);
#pragma unroll
    for (int j = 0; j < 4; j++) xyz[(size_t)4 * i + j] = out[j];
  }
}

}  // namespace

int launch_recover_pose_batch(misift_ctx *ctx, int nsel, const int *h_frames, const float *h_intrinsics,
                              const BatchLayout &set, float min_score, float max_ambiguity, float thresh,
                              const float *F, float *pose, int *num_front, int *votes, float *xyz)
{
  FbPoseArgs B;
  B.set = set;
  B.frames = h_frames; B.K = h_intrinsics;
  B.min_score = min_score; B.max_ambiguity = max_ambiguity; B.thresh2 = thresh * thresh;
  B.F = F; B.pose = pose; B.num_front = num_front; B.votes = votes; B.xyz = xyz;
  LaunchScope ls(ctx, "fund_batch_pose");
  hipLaunchKernelGGL(fund_batch_pose_kernel, dim3(nsel), dim3(POSE_THREADS), 0, ctx->stream, B);
  return ls.finish();
}

// Test-only, host-only: the hypotheses of one F and the depth terms of records under one pose, as the kernel computes
// them (pose_core.hpp).
extern "C" int misift_test_pose_decompose(const float *F9, const float *K8, float *out48, int *valid)
{
  if (!F9 || !K8 || !out48 || !valid) {
    misift_set_error("misift_test_pose_decompose: invalid argument");
    return MISIFT_EINVAL;
  }
  float F[9];
  for (int k = 0; k < 9; k++) F[k] = F9[k];
  const PoseIntrinsics K{K8[0], K8[1], K8[2], K8[3], K8[4], K8[5], K8[6], K8[7]};
  PoseHypotheses h;
  *valid = pose_decompose(F, K, h) ? 1 : 0;
  for (int k = 0; k < 4; k++) {
    float pose[12];
    pose_hypothesis(h, k, pose);
    for (int j = 0; j < 12; j++) out48[12 * k + j] = *valid ? pose[j] : 0.0f;
  }
  return MISIFT_OK;
}

extern "C" int misift_test_pose_vote(const float *pose12, const float *K8, const float *xy, int n,
                                     unsigned char *front_out, float *xyz_out)
{
  if (!pose12 || !K8 || n < 0 || (n > 0 && (!xy || !front_out || !xyz_out))) {
    misift_set_error("misift_test_pose_vote: invalid argument");
    return MISIFT_EINVAL;
  }
  float R[9], t[3];
  for (int j = 0; j < 9; j++) R[j] = pose12[j];
  for (int j = 0; j < 3; j++) t[j] = pose12[9 + j];
  const PoseIntrinsics K{K8[0], K8[1], K8[2], K8[3], K8[4], K8[5], K8[6], K8[7]};
  for (int i = 0; i < n; i++) {
    float p1[3], p2[3], den, n1, n2, out[4];
    pose_normalised(K, xy[4 * i], xy[4 * i + 1], xy[4 * i + 2], xy[4 * i + 3], p1, p2);
    pose_depth_terms(R, t, p1, p2, den, n1, n2);
    front_out[i] = pose_in_front(den, n1, n2) ? 1 : 0;
    pose_xyz(true, den, n1, n2, p1, out);
    for (int j = 0; j < 4; j++) xyz_out[4 * i + j] = out[j];
  }
  return MISIFT_OK;
}
