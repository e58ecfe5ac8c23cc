// kernels_pose_planar.hip — misift_recover_pose_planar_batch: the relative camera pose of the selected frame pairs that
// are planar or rotation-only, from their homographies, behind misift_recover_pose_batch in the chain.  Entry e works on
// frame frames[e] of a device-resident record batch (counts and offsets read on the device) and writes result slot e; no
// host round trip.  No reference counterpart.  The arithmetic is pose_planar_core.hpp, shared with the host-only test
// hooks at the end of this file.
//
// One launch, one 256-thread workgroup per entry, the shape of fund_batch_pose_kernel:
//   count      each thread walks its records r = t, t + 256, ...: the gate, the inlier test under H and, with F, under
//              F.  Integer sums: a wave reduction, then one LDS atomic per wave and count.
//   decompose  thread 0 decides and runs steps 3-6 (A, six Jacobi sweeps, the two solutions, their F): a serial chain
//              that no other lane can shorten.  The hypotheses, 52 floats, go to the others through LDS.  A general or
//              invalid entry ends here, with d_model and d_hf_counts its only outputs.
//   vote       a second walk: two Sampson tests and two depth evaluations per record; -t flips the sign of n1 and n2
//              and nothing else, so the four votes cost two evaluations.  Summed as the counts are.
//   write      the pick's pose, plane and vote, the four votes and the alternative; with d_xyz, a third walk over every
//              record of the frame under the pick.  The records are read again from global memory, all within their
//              first 64 bytes: the frame of a pair is a few hundred KiB at the most and the later walks find it in L2.
#include <math.h>
#include "common.hpp"
#include "pose_planar_core.hpp"

namespace {

constexpr int PLANAR_THREADS = 256;

struct PlanarPoseArgs {
  BatchLayout set;
  const int *frames;                           // pinned host copies of the caller's lists
  const float *K;                              // nsel x 8
  float min_score, max_ambiguity, thresh_h2, thresh_f2, planar_ratio, min_baseline;
  int min_inliers;
  const float *H;                              // nsel x 9
  const float *F;                              // nsel x 9, may be NULL
  int *model;                                  // out: nsel
  int *hf_counts;                              // out: nsel x 2
  float *pose;                                 // out: nsel x 12
  int *num_front;                              // out: nsel
  int *votes;                                  // out: nsel x 4, may be NULL
  float *xyz;                                  // out: 4 floats per record of the batch, may be NULL
  float *pose_alt;                             // out: nsel x 12, may be NULL
  float *plane;                                // out: nsel x 4, may be NULL
};

__device__ __forceinline__ int wave_sum(int v)
{
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(PLANAR_THREADS) void pose_planar_kernel(PlanarPoseArgs B)
{
  __shared__ float s_h[PLANAR_HYP_FLOATS];
  __shared__ int s_model, s_counts[2], s_votes[4];
  const int e = blockIdx.x, f = B.frames[e];
  const int n = max(B.set.counts[f], 0);
  const long long base = B.set.base(f);
  const SiftPointD *pts = B.set.recs + base;
  const bool has_f = B.F != nullptr;
  float H[9], F[9];
#pragma unroll
  for (int k = 0; k < 9; k++) {
    H[k] = B.H[(size_t)9 * e + k];
    F[k] = has_f ? B.F[(size_t)9 * e + k] : 0.0f;
  }
  const float *k8 = B.K + (size_t)8 * e;
  const PoseIntrinsics K{k8[0], k8[1], k8[2], k8[3], k8[4], k8[5], k8[6], k8[7]};
  if (threadIdx.x < 2) s_counts[threadIdx.x] = 0;
  if (threadIdx.x < 4) s_votes[threadIdx.x] = 0;
  __syncthreads();

  int cnt[2] = {0, 0};                         // step 1
  for (int i = threadIdx.x; i < n; i += PLANAR_THREADS) {
    const SiftPointD &pt = pts[i];
    const float x1 = pt.xpos, y1 = pt.ypos, x2 = pt.match_xpos, y2 = pt.match_ypos;
    if (!(pt.score > B.min_score && pt.ambiguity < B.max_ambiguity)) continue;
    cnt[0] += planar_h_inlier(H, x1, y1, x2, y2, B.thresh_h2) ? 1 : 0;
    if (has_f) {
      float sden;
      const float e2 = fundamental_sampson(F, x1, y1, x2, y2, sden);
      cnt[1] += fundamental_inlier(e2, sden, B.thresh_f2) ? 1 : 0;
    }
  }
#pragma unroll
  for (int k = 0; k < 2; k++) {
    cnt[k] = wave_sum(cnt[k]);
    if ((threadIdx.x & 63) == 0 && cnt[k]) atomicAdd(&s_counts[k], cnt[k]);
  }
  __syncthreads();

  PlanarHypotheses h;
  if (threadIdx.x == 0) {                      // steps 2-6
    const int nH = s_counts[0], nF = s_counts[1];
    int model = PLANAR_GENERAL;
    if (planar_candidate(nH, nF, has_f, B.min_inliers, B.planar_ratio)) model = planar_decompose(H, K, B.min_baseline, h);
    s_model = model;
    B.model[e] = model;
    B.hf_counts[(size_t)2 * e] = nH;
    B.hf_counts[(size_t)2 * e + 1] = nF;
    if (model > 0) {
      float a[PLANAR_HYP_FLOATS];
      planar_pack(h, a);
#pragma unroll
      for (int j = 0; j < PLANAR_HYP_FLOATS; j++) s_h[j] = a[j];
    }
  }
  __syncthreads();
  const int model = s_model;
  if (model <= 0) return;                      // general or invalid: nothing else is written
  {
    float a[PLANAR_HYP_FLOATS];
#pragma unroll
    for (int j = 0; j < PLANAR_HYP_FLOATS; j++) a[j] = s_h[j];
    planar_unpack(a, h);
  }

  float pose[12], plane[4];
  if (model == PLANAR_ROTATION) {              // step 5: R, t = 0, no vote, no plane, no depth
#pragma unroll
    for (int j = 0; j < 12; j++) pose[j] = j < 9 ? h.Ra[j] : 0.0f;
    if (threadIdx.x == 0) {
#pragma unroll
      for (int j = 0; j < 12; j++) {
        B.pose[(size_t)12 * e + j] = pose[j];
        if (B.pose_alt) B.pose_alt[(size_t)12 * e + j] = pose[j];
      }
      B.num_front[e] = 0;
    }
    if (threadIdx.x < 4) {
      if (B.votes) B.votes[(size_t)4 * e + threadIdx.x] = 0;
      if (B.plane) B.plane[(size_t)4 * e + threadIdx.x] = 0.0f;
    }
  } else {
    int v[4] = {0, 0, 0, 0};                   // step 7
    for (int i = threadIdx.x; i < n; i += PLANAR_THREADS) {
      const SiftPointD &pt = pts[i];
      if (!(pt.score > B.min_score && pt.ambiguity < B.max_ambiguity)) continue;
      bool rv[4];
      planar_record_votes(h, K, pt.xpos, pt.ypos, pt.match_xpos, pt.match_ypos, B.thresh_f2, rv);
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] += rv[k] ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      v[k] = wave_sum(v[k]);
      if ((threadIdx.x & 63) == 0 && v[k]) atomicAdd(&s_votes[k], v[k]);
    }
    __syncthreads();
    const int votes[4] = {s_votes[0], s_votes[1], s_votes[2], s_votes[3]};
    int best, alt;
    planar_pick(votes, best, alt);
    planar_hypothesis(h, best, pose, plane);
    if (threadIdx.x == 0) {
      float pose_alt[12], plane_alt[4];
      planar_hypothesis(h, alt, pose_alt, plane_alt);
#pragma unroll
      for (int j = 0; j < 12; j++) {
        B.pose[(size_t)12 * e + j] = pose[j];
        if (B.pose_alt) B.pose_alt[(size_t)12 * e + j] = pose_alt[j];
      }
      B.num_front[e] = best == 0 ? votes[0] : (best == 1 ? votes[1] : (best == 2 ? votes[2] : votes[3]));
    }
    if (threadIdx.x < 4) {
      if (B.votes) B.votes[(size_t)4 * e + threadIdx.x] = s_votes[threadIdx.x];
      if (B.plane) {
        const float p = threadIdx.x == 0 ? plane[0] : (threadIdx.x == 1 ? plane[1] : (threadIdx.x == 2 ? plane[2] : plane[3]));
        B.plane[(size_t)4 * e + threadIdx.x] = p;
      }
    }
  }
  if (!B.xyz) return;                          // step 8
  float R[9], t[3];
#pragma unroll
  for (int j = 0; j < 9; j++) R[j] = pose[j];
#pragma unroll
  for (int j = 0; j < 3; j++) t[j] = pose[9 + j];
  float *xyz = B.xyz + (size_t)base * 4;
  for (int i = threadIdx.x; i < n; i += PLANAR_THREADS) {
    const SiftPointD &pt = pts[i];
    float p1[3], p2[3], den, n1, n2, out[4];
    pose_normalised(K, pt.xpos, pt.ypos, pt.match_xpos, pt.match_ypos, p1, p2);
    pose_depth_terms(R, t, p1, p2, den, n1, n2);
    pose_xyz(model == PLANAR_PLANE, den, n1, n2, p1, out);
#pragma unroll
    for (int j = 0; j < 4; j++) xyz[(size_t)4 * i + j] = out[j];
  }
}

}  // namespace

int launch_recover_pose_planar_batch(misift_ctx *ctx, int nsel, const int *h_frames, const float *h_intrinsics,
                                     const BatchLayout &set, const PlanarPoseParams &p, const float *H, const float *F,
                                     const PlanarPoseOut &out)
{
  PlanarPoseArgs B;
  B.set = set;
  B.frames = h_frames; B.K = h_intrinsics;
  B.min_score = p.min_score; B.max_ambiguity = p.max_ambiguity;
  B.thresh_h2 = p.thresh_h * p.thresh_h; B.thresh_f2 = p.thresh_f * p.thresh_f;
  B.planar_ratio = p.planar_ratio; B.min_baseline = p.min_baseline; B.min_inliers = p.min_inliers;
  B.H = H; B.F = F;
  B.model = out.model; B.hf_counts = out.hf_counts; B.pose = out.pose; B.num_front = out.num_front;
  B.votes = out.votes; B.xyz = out.xyz; B.pose_alt = out.pose_alt; B.plane = out.plane;
  LaunchScope ls(ctx, "pose_planar");
  hipLaunchKernelGGL(pose_planar_kernel, dim3(nsel), dim3(PLANAR_THREADS), 0, ctx->stream, B);
  return ls.finish();
}

// Test-only, host-only: steps 3-6 with the two F of step 7, and steps 1, 2 and 7 (per record, then the counts, the
// decision and the pick), as the kernel computes them (pose_planar_core.hpp).
extern "C" int misift_test_pose_planar_decompose(const float *H9, const float *K8, float min_baseline, float *out84,
                                                 int *model)
{
  if (!H9 || !K8 || !out84 || !model) {
    misift_set_error("misift_test_pose_planar_decompose: invalid argument");
    return MISIFT_EINVAL;
  }
  return planar_hook_decompose(H9, K8, min_baseline, out84, model);
}

extern "C" int misift_test_pose_planar_vote(const float *H9, const float *F9, const float *hyp84, const float *K8,
                                            const float *xy, const unsigned char *gate, int n, float thresh_h,
                                            float thresh_f, float planar_ratio, int min_inliers, unsigned char *h_in,
                                            unsigned char *f_in, unsigned char *votes, int *decision9)
{
  if (!H9 || !hyp84 || !K8 || !decision9 || n < 0 || (n > 0 && (!xy || !gate || !h_in || !f_in || !votes))) {
    misift_set_error("misift_test_pose_planar_vote: invalid argument");
    return MISIFT_EINVAL;
  }
  return planar_hook_vote(H9, F9, hyp84, K8, xy, gate, n, thresh_h, thresh_f, planar_ratio, min_inliers, h_in, f_in, votes,
                          decision9);
}
