// bundle_core.hpp — the arithmetic of misift_adjust_bundle_batch, for host and device: every phase of the call as a
// function of one work item (a slot, a track, an image) over a BundleData, a struct of plain pointers.  The kernels
// (kernels_bundle.hip) hand in the call's arguments and temp memory and run one work item per lane or per workgroup; the
// host-only test hook (misift_test_adjust_bundle) hands in host arrays and runs the same functions in loops, phase after
// phase in the order of the launches.  So what a CPU test pins is what the device runs.  The definition, step by step,
// is in include/misift.h.  misift_adjust_bundle_robust_batch is the same call with a loss: bundle_loss gives rho, w and
// sqrt(w) of a member's squared residual, step 1 scales the member's 20 values by sqrt(w) where it writes them, the cost
// pass stores rho in place of the squared residual, and every phase downstream reads what those two wrote.  ROBUST is a
// template argument of the two, so the plain call compiles to what it was.
//
// The rules of refine_core.hpp hold: fp32 with every operation rounded, only + - * / sqrtf and fabsf, no fmaf, and the
// build's -ffp-contract=off.  A per-track sum is taken by one work item in ascending slot.  A per-image or cross-image
// sum is the 256-slot rule of fundamental_core.hpp (fundamental_slot_partial, then the halving tree) over the position
// in the image's member list, or over the image index; how the 256 partial sums are spread is the Sum's business: the
// kernel's workgroup (thread s = slot s, the tree through LDS) or the hook's loop.  A Sum has
//   template <int K, class V> void sum(int n, V &v, float (&out)[K]);   the same values in every thread that runs it
#pragma once
#include <math.h>
#include "refine_core.hpp"

enum { BUNDLE_ADJUSTED = 0, BUNDLE_FEW_OBS = 1, BUNDLE_HELD = 3, BUNDLE_NO_CAMERA = 4 };
enum { BUNDLE_CUR = 0, BUNDLE_FAIL = 1, BUNDLE_BAD = 2, BUNDLE_ALIVE = 3, BUNDLE_ITERS = 4, BUNDLE_KEPT = 5,
       BUNDLE_STEP = 6, BUNDLE_CTL = 8 };
enum { BUNDLE_LAM = 0, BUNDLE_COST = 1, BUNDLE_RHO = 2, BUNDLE_COST0 = 3, BUNDLE_FCTL = 4 };
constexpr int BUNDLE_LIN = 20;                 // per slot: Ju_c (6), Jv_c (6), Ju_p (3), Jv_p (3), ru, rv
constexpr int BUNDLE_NORMAL = 33;              // per image: U (21, row-major upper triangle), gc (6), sum of W y (6)
constexpr float BUNDLE_LAMBDA_FLOOR = 1e-7f;   // below it 1 + lambda is 1 in fp32
enum { BUNDLE_LOSS_NONE = 0, BUNDLE_LOSS_HUBER = 1, BUNDLE_LOSS_GEMAN_MCCLURE = 2 };   // MISIFT_LOSS_*

struct BundleData {
  TrackScene s;                                // the call's inputs
  int min_views, min_obs, num_loops, cg_iters, orthonormalise;
  float thresh2, lambda0;
  int loss;                                    // BUNDLE_LOSS_*, the same for the whole call
  float loss_scale, loss_scale2;               // c, and c*c rounded once on the host; not read with loss 0
  const int *held;                             // nimages flags
  // temp
  int *owner, *key, *list;                     // max_obs each; key[o] = the image slot o is a member of, or -1
  int *istart, *icount, *istate;               // nimages each: the image's run of `list`, its status
  int *tcount;                                 // max_tracks: the pre-members of the track
  int *ctl;                                    // BUNDLE_CTL
  float *fctl;                                 // BUNDLE_FCTL
  float *lin;                                  // max_obs x BUNDLE_LIN
  float *eterm;                                // 2 x max_obs: ru^2 + rv^2 under state buffer b
  float *cams;                                 // 2 x nimages x 12: the two state buffers
  float *pts;                                  // 2 x max_tracks x 3
  float *tv;                                   // max_tracks x 9: V' (m00 m01 m02 m11 m12 m22), gp
  float *tq;                                   // max_tracks x 3: V'^-1 gp, then q_t of each CG iteration
  float *iu;                                   // nimages x 28: [1..21] U', [22..27] b, as refine_solve reads them
  float *ivec;                                 // 5 x nimages x 6: x, r, z, p, y
  float *icost;                                // 3 x nimages: at the start, of the state, of the trial state
  // outputs
  float *cam_out, *points_out, *cam_rms, *history, *cost;
  int *cam_obs, *cam_status, *point_obs, *summary;
  float *obs_weight;                           // max_obs, or NULL
};

FUND_HD void bundle_raise(int *flag)
{
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(flag, 1);
#else
  *flag |= 1;
#endif
}
FUND_HD void bundle_count(int *sum, int v)
{
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(sum, v);
#else
  *sum += v;
#endif
}

FUND_HD float bundle_dot6(const float *a, const float *b)
{
  return ((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5];
}

FUND_HD float *bundle_vec(const BundleData &D, int which, int i) { return D.ivec + 6 * ((size_t)which * D.s.nimages + i); }
enum { BUNDLE_X = 0, BUNDLE_R = 1, BUNDLE_Z = 2, BUNDLE_P = 3, BUNDLE_Y = 4 };

FUND_HD void bundle_load_cam(const float *src, float (&c)[12])
{
#pragma unroll
  for (int j = 0; j < 12; j++) c[j] = src[j];
}

// ---- the sets, decided once

// an image's state and the camera both state buffers start with
FUND_HD void bundle_image_init(const BundleData &D, int i)
{
  float c[12];
  bundle_load_cam(D.s.cam + 12 * (size_t)i, c);
  const int pair = D.s.cam_pair[i];
  int state = BUNDLE_ADJUSTED;
  if (pair == POSEGRAPH_UNSET || !refine_finite12(c)) state = BUNDLE_NO_CAMERA;
  else if (pair == POSEGRAPH_ROOT || D.held[i] != 0) state = BUNDLE_HELD;
  else if (D.orthonormalise) {
    float o[12];
    bundle_load_cam(D.s.cam + 12 * (size_t)i, o);
    if (refine_orthonormalise(o)) {
#pragma unroll
      for (int j = 0; j < 12; j++) c[j] = o[j];
    } else {
      state = BUNDLE_NO_CAMERA;
    }
  }
  D.istate[i] = state;
#pragma unroll
  for (int j = 0; j < 12; j++) {
    D.cams[12 * (size_t)i + j] = c[j];
    D.cams[12 * ((size_t)D.s.nimages + i) + j] = c[j];
  }
}

// slot o < O: a candidate stays in `key` iff it is a pre-member
FUND_HD void bundle_slot_premember(const BundleData &D, int o)
{
  const int k = D.key[o];
  if (k < 0) return;
  bool in = D.istate[k] != BUNDLE_NO_CAMERA;
  if (in) {
    float c[12];
    bundle_load_cam(D.cams + 12 * (size_t)k, c);
    const float *P = D.s.points + 4 * (size_t)D.owner[o];
    const float X[3] = {P[0], P[1], P[2]};
    const TrackObs ob = track_obs_load(D.s.obs + o);
    in = refine_member(c, D.s.intrinsics + 4 * (size_t)k, X, ob.xpos, ob.ypos, D.thresh2);
  }
  if (!in) D.key[o] = -1;
}

// track t < T: its pre-members counted; an inactive track's leave `key`, an active track's point enters both buffers
FUND_HD void bundle_track_activate(const BundleData &D, int t)
{
  const int off = D.s.track_offsets[t], end = D.s.track_offsets[t + 1];
  int n = 0;
  const bool valid = tri_range_ok(off, end, scene_O(D.s));
  if (valid)
    for (int o = off; o < end; o++) n += (D.owner[o] == t && D.key[o] >= 0) ? 1 : 0;
  D.tcount[t] = n;
  if (!valid) return;
  if (n < D.min_views) {
    for (int o = off; o < end; o++)
      if (D.owner[o] == t) D.key[o] = -1;
    return;
  }
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const float v = D.s.points[4 * (size_t)t + j];
    D.pts[3 * (size_t)t + j] = v;
    D.pts[3 * ((size_t)D.s.max_tracks + t) + j] = v;
  }
}

FUND_HD bool bundle_active(const BundleData &D, int t) { return D.tcount[t] >= D.min_views; }

// ---- one member under a state

// step 1: Jc, Jp and r of a member; false when it is not in front
FUND_HD bool bundle_linearise(const float (&c)[12], const float *k, const float (&X)[3], float x, float y,
                              float (&l)[BUNDLE_LIN])
{
  RefineView v;
  if (!refine_view(c, k, X, x, y, v)) return false;
  const float gx = k[0] * v.iz, gy = k[1] * v.iz;
  l[0] = gx * -(v.a * v.yc); l[1] = gx * (v.zc + v.a * v.xc); l[2] = gx * -v.yc;
  l[3] = gx * 1.0f; l[4] = gx * 0.0f; l[5] = gx * -v.a;
  l[6] = gy * -(v.zc + v.b * v.yc); l[7] = gy * (v.b * v.xc); l[8] = gy * v.xc;
  l[9] = gy * 0.0f; l[10] = gy * 1.0f; l[11] = gy * -v.b;
  l[12] = gx * (c[0] - v.a * c[6]); l[13] = gx * (c[1] - v.a * c[7]); l[14] = gx * (c[2] - v.a * c[8]);
  l[15] = gy * (c[3] - v.b * c[6]); l[16] = gy * (c[4] - v.b * c[7]); l[17] = gy * (c[5] - v.b * c[8]);
  l[18] = v.ru;
  l[19] = v.rv;
  return true;
}

// W[r][q] = Ju_c[r]*Ju_p[q] + Jv_c[r]*Jv_p[q]
FUND_HD float bundle_w(const float *l, int r, int q) { return l[r] * l[12 + q] + l[6 + r] * l[15 + q]; }
// (W v)[r] for a 3-vector v, (W^T v)[q] for a 6-vector v
FUND_HD float bundle_w3(const float *l, int r, const float *v)
{
  return (bundle_w(l, r, 0) * v[0] + bundle_w(l, r, 1) * v[1]) + bundle_w(l, r, 2) * v[2];
}
FUND_HD float bundle_wt6(const float *l, int q, const float *v)
{
  return ((((bundle_w(l, 0, q) * v[0] + bundle_w(l, 1, q) * v[1]) + bundle_w(l, 2, q) * v[2]) + bundle_w(l, 3, q) * v[3]) +
          bundle_w(l, 4, q) * v[4]) + bundle_w(l, 5, q) * v[5];
}

// the loss of a member: rho, w and sw = sqrt(w) of s = ru*ru + rv*rv
struct BundleLoss {
  float rho, w, sw;
};
FUND_HD BundleLoss bundle_loss(int loss, float c, float c2, float s)
{
  BundleLoss L;
  L.rho = s;
  L.w = L.sw = 1.0f;
  if (loss == BUNDLE_LOSS_HUBER) {
    if (!(s <= c2)) {                          // a NaN s comes here
      const float n = sqrtf(s);
      L.rho = (c + c) * n - c2;
      L.w = c / n;
      L.sw = sqrtf(L.w);
    }
  } else if (loss == BUNDLE_LOSS_GEMAN_MCCLURE) {
    const float d = c2 + s, q = c2 / d;
    L.rho = (s * c2) / d;
    L.w = q * q;
    L.sw = q;
  }
  return L;
}

// a member's squared residual, or its rho, under state buffer b (trial: the buffer the state is not in); one not in front raises BAD
template <bool ROBUST>
FUND_HD void bundle_eval_slot(const BundleData &D, int o, bool trial)
{
  const int k = D.key[o];
  if (k < 0) return;
  if (trial && D.ctl[BUNDLE_FAIL]) return;
  const int b = trial ? 1 - D.ctl[BUNDLE_CUR] : D.ctl[BUNDLE_CUR];
  float c[12];
  bundle_load_cam(D.cams + 12 * ((size_t)b * D.s.nimages + k), c);
  const float *P = D.pts + 3 * ((size_t)b * D.s.max_tracks + D.owner[o]);
  const float X[3] = {P[0], P[1], P[2]};
  const TrackObs ob = track_obs_load(D.s.obs + o);
  RefineView v;
  float e = 0.0f;
  if (refine_view(c, D.s.intrinsics + 4 * (size_t)k, X, ob.xpos, ob.ypos, v)) {
    e = v.ru * v.ru + v.rv * v.rv;
    if (ROBUST) e = bundle_loss(D.loss, D.loss_scale, D.loss_scale2, e).rho;
  } else {
    bundle_raise(&D.ctl[BUNDLE_BAD]);
  }
  D.eterm[(size_t)b * D.s.max_obs + o] = e;
}

// an image's cost under that buffer: the position rule over its list
struct BundleCostTerm {
  const float *e;
  const int *list;
  FUND_HD bool operator()(int p, float (&x)[1]) const { x[0] = e[list[p]]; return true; }
};
template <class Sum>
FUND_HD void bundle_image_cost(const BundleData &D, Sum &S, int i, bool trial, bool lead)
{
  if (trial && D.ctl[BUNDLE_FAIL]) return;
  const int b = trial ? 1 - D.ctl[BUNDLE_CUR] : D.ctl[BUNDLE_CUR];
  BundleCostTerm term{D.eterm + (size_t)b * D.s.max_obs, D.list + D.istart[i]};
  float c[1];
  S.template sum<1>(D.icount[i], term, c);
  if (!lead) return;
  if (trial) D.icost[2 * (size_t)D.s.nimages + i] = c[0];
  else D.icost[i] = D.icost[(size_t)D.s.nimages + i] = c[0];
}

// a cross-image sum: the 256-slot rule over the image index
struct BundleImageCostTerm {
  const float *c;
  FUND_HD bool operator()(int i, float (&x)[1]) const { x[0] = c[i]; return true; }
};
struct BundleDotTerm {
  const int *istate;
  const float *a, *b;
  FUND_HD bool operator()(int i, float (&x)[1]) const
  {
    if (istate[i] != BUNDLE_ADJUSTED) return false;
    x[0] = bundle_dot6(a + 6 * (size_t)i, b + 6 * (size_t)i);
    return true;
  }
};

// the scalar workgroup at the start: the cost of the starting state, lambda0, the flags cleared; lead: the thread that
// writes the scalars.  Below, `lane` and `lanes` say which images a thread of that workgroup takes: lane + j*lanes
template <class Sum>
FUND_HD void bundle_scalar_init(const BundleData &D, Sum &S, bool lead)
{
  BundleImageCostTerm term{D.icost};
  float c[1];
  S.template sum<1>(D.s.nimages, term, c);
  if (!lead) return;
  for (int j = 0; j < BUNDLE_CTL; j++) D.ctl[j] = 0;
  D.fctl[BUNDLE_LAM] = D.lambda0;
  D.fctl[BUNDLE_COST] = D.fctl[BUNDLE_COST0] = c[0];
  D.fctl[BUNDLE_RHO] = 0.0f;
}

// ---- one LM step

// step 1 and 2 for an active track: its members linearised under the state (ROBUST: each of the 20 values times sw,
// s taken from the unscaled ru, rv), V, gp, V' and V'^-1 gp
template <bool ROBUST>
FUND_HD void bundle_track_normal(const BundleData &D, int t)
{
  if (!bundle_active(D, t)) return;
  const int b = D.ctl[BUNDLE_CUR];
  const float lam1 = 1.0f + D.fctl[BUNDLE_LAM];
  const float *P = D.pts + 3 * ((size_t)b * D.s.max_tracks + t);
  const float X[3] = {P[0], P[1], P[2]};
  TriNormal N;
  tri_clear(N);
  const int off = D.s.track_offsets[t], end = D.s.track_offsets[t + 1];
  for (int o = off; o < end; o++) {
    const int k = D.key[o];
    if (D.owner[o] != t || k < 0) continue;
    float c[12], l[BUNDLE_LIN];
    bundle_load_cam(D.cams + 12 * ((size_t)b * D.s.nimages + k), c);
    const TrackObs ob = track_obs_load(D.s.obs + o);
    if (!bundle_linearise(c, D.s.intrinsics + 4 * (size_t)k, X, ob.xpos, ob.ypos, l)) {
      bundle_raise(&D.ctl[BUNDLE_FAIL]);       // the state has every member in front: not reached
#pragma unroll
      for (int j = 0; j < BUNDLE_LIN; j++) l[j] = 0.0f;
    }
    if (ROBUST) {
      const float sw = bundle_loss(D.loss, D.loss_scale, D.loss_scale2, l[18] * l[18] + l[19] * l[19]).sw;
#pragma unroll
      for (int j = 0; j < BUNDLE_LIN; j++) l[j] = sw * l[j];
    }
    float *dst = D.lin + (size_t)BUNDLE_LIN * o;
#pragma unroll
    for (int j = 0; j < BUNDLE_LIN; j++) dst[j] = l[j];
    tri_accumulate(N, l[12], l[13], l[14], l[18]);
    tri_accumulate(N, l[15], l[16], l[17], l[19]);
  }
  N.m00 = N.m00 * lam1; N.m11 = N.m11 * lam1; N.m22 = N.m22 * lam1;
  float y[3];
  if (!tri_solve(N, y)) bundle_raise(&D.ctl[BUNDLE_FAIL]);
  float *v = D.tv + 9 * (size_t)t, *q = D.tq + 3 * (size_t)t;
  v[0] = N.m00; v[1] = N.m01; v[2] = N.m02; v[3] = N.m11; v[4] = N.m12; v[5] = N.m22;
  v[6] = N.g0; v[7] = N.g1; v[8] = N.g2;
  q[0] = y[0]; q[1] = y[1]; q[2] = y[2];
}

// V'^-1 rhs for track t; a failed solve gives zeros
FUND_HD void bundle_track_solve(const BundleData &D, int t, const float (&rhs)[3], float (&x)[3])
{
  const float *v = D.tv + 9 * (size_t)t;
  TriNormal N;
  N.m00 = v[0]; N.m01 = v[1]; N.m02 = v[2]; N.m11 = v[3]; N.m12 = v[4]; N.m22 = v[5];
  N.g0 = rhs[0]; N.g1 = rhs[1]; N.g2 = rhs[2];
  tri_solve(N, x);
}

// sum over the track's members in free images, in ascending slot, of W^T v_image; v = the 6-vectors `which`
FUND_HD void bundle_track_gather(const BundleData &D, int t, int which, float (&s)[3])
{
  s[0] = s[1] = s[2] = 0.0f;
  const int off = D.s.track_offsets[t], end = D.s.track_offsets[t + 1];
  for (int o = off; o < end; o++) {
    const int k = D.key[o];
    if (D.owner[o] != t || k < 0 || D.istate[k] != BUNDLE_ADJUSTED) continue;
    const float *l = D.lin + (size_t)BUNDLE_LIN * o, *v = bundle_vec(D, which, k);
#pragma unroll
    for (int q = 0; q < 3; q++) s[q] = s[q] + bundle_wt6(l, q, v);
  }
}

// step 3 for a free image: U, gc and the sum of W (V'^-1 gp) by the position rule; U', b
struct BundleNormalTerm {
  const BundleData &D;
  const int *list;
  FUND_HD bool operator()(int p, float (&x)[BUNDLE_NORMAL]) const
  {
    const int o = list[p];
    const float *l = D.lin + (size_t)BUNDLE_LIN * o, *y = D.tq + 3 * (size_t)D.owner[o];
    int i = 0;
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
      for (int c = r; c < 6; c++) x[i++] = l[r] * l[c] + l[6 + r] * l[6 + c];
#pragma unroll
    for (int r = 0; r < 6; r++) x[21 + r] = l[r] * l[18] + l[6 + r] * l[19];
#pragma unroll
    for (int r = 0; r < 6; r++) x[27 + r] = bundle_w3(l, r, y);
    return true;
  }
};
template <class Sum>
FUND_HD void bundle_image_normal(const BundleData &D, Sum &S, int i, bool lead)
{
  if (D.istate[i] != BUNDLE_ADJUSTED) return;
  BundleNormalTerm term{D, D.list + D.istart[i]};
  float s[BUNDLE_NORMAL];
  S.template sum<BUNDLE_NORMAL>(D.icount[i], term, s);
  if (!lead) return;
  const float lam1 = 1.0f + D.fctl[BUNDLE_LAM];
  float R[REFINE_SUMS], delta[6];
  R[0] = 0.0f;
  int j = 0;
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int c = r; c < 6; c++) {
      R[1 + j] = r == c ? s[j] * lam1 : s[j];
      j++;
    }
#pragma unroll
  for (int r = 0; r < 6; r++) R[22 + r] = s[21 + r] - s[27 + r];
  if (!refine_solve(R, delta)) bundle_raise(&D.ctl[BUNDLE_FAIL]);
  float *dst = D.iu + (size_t)REFINE_SUMS * i;
#pragma unroll
  for (int r = 0; r < REFINE_SUMS; r++) dst[r] = R[r];
}

// M^-1 v for image i (the LDL^T of U'); a failed solve gives zeros
FUND_HD void bundle_precondition(const BundleData &D, int i, const float *v, float *z)
{
  float R[REFINE_SUMS], delta[6];
  const float *src = D.iu + (size_t)REFINE_SUMS * i;
#pragma unroll
  for (int r = 0; r < 22; r++) R[r] = src[r];
#pragma unroll
  for (int r = 0; r < 6; r++) R[22 + r] = v[r];
  refine_solve(R, delta);
#pragma unroll
  for (int r = 0; r < 6; r++) z[r] = delta[r];
}

// step 4, the start of PCG in the scalar workgroup; this thread takes the images lane, lane + lanes, ...
template <class Sum>
FUND_HD void bundle_cg_start(const BundleData &D, Sum &S, int lane, int lanes, bool lead)
{
  const bool fail = D.ctl[BUNDLE_FAIL] != 0;
  for (int i = lane; i < D.s.nimages; i += lanes) {
    if (D.istate[i] != BUNDLE_ADJUSTED) continue;
    float *x = bundle_vec(D, BUNDLE_X, i), *r = bundle_vec(D, BUNDLE_R, i), *z = bundle_vec(D, BUNDLE_Z, i),
          *p = bundle_vec(D, BUNDLE_P, i);
    for (int j = 0; j < 6; j++) x[j] = 0.0f;
    if (fail) continue;
    for (int j = 0; j < 6; j++) r[j] = D.iu[(size_t)REFINE_SUMS * i + 22 + j];
    bundle_precondition(D, i, r, z);
    for (int j = 0; j < 6; j++) p[j] = z[j];
  }
  float rho[1] = {0.0f};
  if (!fail) {                                 // the same in every thread
    S.fence();
    BundleDotTerm term{D.istate, D.ivec + 6 * (size_t)BUNDLE_R * D.s.nimages, D.ivec + 6 * (size_t)BUNDLE_Z * D.s.nimages};
    S.template sum<1>(D.s.nimages, term, rho);
  }
  if (!lead) return;
  D.fctl[BUNDLE_RHO] = rho[0];
  D.ctl[BUNDLE_ALIVE] = (!fail && fundamental_finite(rho[0])) ? 1 : 0;
  D.ctl[BUNDLE_ITERS] = 0;
}

// a CG iteration, per active track: q_t = V'^-1 sum W^T p_image
FUND_HD void bundle_cg_track(const BundleData &D, int t)
{
  if (!D.ctl[BUNDLE_ALIVE] || !bundle_active(D, t)) return;
  float s[3], q[3];
  bundle_track_gather(D, t, BUNDLE_P, s);
  bundle_track_solve(D, t, s, q);
  float *dst = D.tq + 3 * (size_t)t;
  dst[0] = q[0]; dst[1] = q[1]; dst[2] = q[2];
}

// a CG iteration, per free image: y_i = U' p_i - sum W q_t
struct BundleWqTerm {
  const BundleData &D;
  const int *list;
  FUND_HD bool operator()(int p, float (&x)[6]) const
  {
    const int o = list[p];
    const float *l = D.lin + (size_t)BUNDLE_LIN * o, *q = D.tq + 3 * (size_t)D.owner[o];
#pragma unroll
    for (int r = 0; r < 6; r++) x[r] = bundle_w3(l, r, q);
    return true;
  }
};
template <class Sum>
FUND_HD void bundle_cg_image(const BundleData &D, Sum &S, int i, bool lead)
{
  if (!D.ctl[BUNDLE_ALIVE] || D.istate[i] != BUNDLE_ADJUSTED) return;
  BundleWqTerm term{D, D.list + D.istart[i]};
  float s[6];
  S.template sum<6>(D.icount[i], term, s);
  if (!lead) return;
  const float *src = D.iu + (size_t)REFINE_SUMS * i, *p = bundle_vec(D, BUNDLE_P, i);
  float U[6][6];
  int j = 1;
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int c = r; c < 6; c++) {
      U[r][c] = U[c][r] = src[j];
      j++;
    }
  float *y = bundle_vec(D, BUNDLE_Y, i);
#pragma unroll
  for (int r = 0; r < 6; r++) y[r] = bundle_dot6(U[r], p) - s[r];
}

// a CG iteration in the scalar workgroup: sigma, alpha, x, r, z, rho', beta, p
template <class Sum>
FUND_HD void bundle_cg_scalar(const BundleData &D, Sum &S, int lane, int lanes, bool lead)
{
  if (!D.ctl[BUNDLE_ALIVE]) return;            // the same in every thread
  const float rho = D.fctl[BUNDLE_RHO];
  const size_t n6 = 6 * (size_t)D.s.nimages;
  BundleDotTerm sterm{D.istate, D.ivec + BUNDLE_P * n6, D.ivec + BUNDLE_Y * n6};
  float sigma[1], rho2[1];
  S.template sum<1>(D.s.nimages, sterm, sigma);
  if (!(fundamental_finite(sigma[0]) && sigma[0] > 0.0f)) {
    S.fence();                                 // every thread has read ALIVE
    if (lead) D.ctl[BUNDLE_ALIVE] = 0;
    return;
  }
  const float alpha = rho / sigma[0];
  for (int i = lane; i < D.s.nimages; i += lanes) {
    if (D.istate[i] != BUNDLE_ADJUSTED) continue;
    float *x = bundle_vec(D, BUNDLE_X, i), *r = bundle_vec(D, BUNDLE_R, i), *z = bundle_vec(D, BUNDLE_Z, i);
    const float *p = bundle_vec(D, BUNDLE_P, i), *y = bundle_vec(D, BUNDLE_Y, i);
    for (int j = 0; j < 6; j++) x[j] = x[j] + alpha * p[j];
    for (int j = 0; j < 6; j++) r[j] = r[j] - alpha * y[j];
    bundle_precondition(D, i, r, z);
  }
  S.fence();
  BundleDotTerm rterm{D.istate, D.ivec + BUNDLE_R * n6, D.ivec + BUNDLE_Z * n6};
  S.template sum<1>(D.s.nimages, rterm, rho2);
  const bool on = fundamental_finite(rho2[0]);
  if (on) {
    const float beta = rho2[0] / rho;
    for (int i = lane; i < D.s.nimages; i += lanes) {
      if (D.istate[i] != BUNDLE_ADJUSTED) continue;
      float *p = bundle_vec(D, BUNDLE_P, i);
      const float *z = bundle_vec(D, BUNDLE_Z, i);
      for (int j = 0; j < 6; j++) p[j] = z[j] + beta * p[j];
    }
  }
  S.fence();
  if (!lead) return;
  D.ctl[BUNDLE_ITERS] = D.ctl[BUNDLE_ITERS] + 1;
  if (on) D.fctl[BUNDLE_RHO] = rho2[0];
  else D.ctl[BUNDLE_ALIVE] = 0;
}

// step 5 for an active track: delta_t = V'^-1 (gp - sum W^T x_image), the trial point
FUND_HD void bundle_track_trial(const BundleData &D, int t)
{
  if (D.ctl[BUNDLE_FAIL] || !bundle_active(D, t)) return;
  const int b = D.ctl[BUNDLE_CUR];
  float s[3], d[3];
  bundle_track_gather(D, t, BUNDLE_X, s);
  const float *v = D.tv + 9 * (size_t)t;
  const float rhs[3] = {v[6] - s[0], v[7] - s[1], v[8] - s[2]};
  bundle_track_solve(D, t, rhs, d);
  const float *X = D.pts + 3 * ((size_t)b * D.s.max_tracks + t);
  float *Y = D.pts + 3 * ((size_t)(1 - b) * D.s.max_tracks + t);
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const float e = X[j] + d[j];
    Y[j] = e;
    ok = ok && fundamental_finite(e);
  }
  if (!ok) bundle_raise(&D.ctl[BUNDLE_BAD]);
}

// step 5 for a free image: the trial camera by the Cayley update
FUND_HD void bundle_image_trial(const BundleData &D, int i)
{
  if (D.ctl[BUNDLE_FAIL] || D.istate[i] != BUNDLE_ADJUSTED) return;
  const int b = D.ctl[BUNDLE_CUR];
  float c[12], out[12], x[6];
  bundle_load_cam(D.cams + 12 * ((size_t)b * D.s.nimages + i), c);
#pragma unroll
  for (int j = 0; j < 6; j++) x[j] = bundle_vec(D, BUNDLE_X, i)[j];
  refine_update(c, x, out);
  float *dst = D.cams + 12 * ((size_t)(1 - b) * D.s.nimages + i);
#pragma unroll
  for (int j = 0; j < 12; j++) dst[j] = out[j];
  if (!refine_finite12(out)) bundle_raise(&D.ctl[BUNDLE_BAD]);
}

// step 6 in the scalar workgroup
template <class Sum>
FUND_HD void bundle_decide(const BundleData &D, Sum &S, int lane, int lanes, bool lead)
{
  const bool broken = D.ctl[BUNDLE_FAIL] != 0 || D.ctl[BUNDLE_BAD] != 0;   // the same in every thread
  const float c = D.fctl[BUNDLE_COST], lam = D.fctl[BUNDLE_LAM];
  float c2[1] = {0.0f};
  if (!broken) {
    BundleImageCostTerm term{D.icost + 2 * (size_t)D.s.nimages};
    S.template sum<1>(D.s.nimages, term, c2);
  }
  const bool kept = !broken && c2[0] < c;
  if (kept)
    for (int i = lane; i < D.s.nimages; i += lanes) D.icost[(size_t)D.s.nimages + i] = D.icost[2 * (size_t)D.s.nimages + i];
  S.fence();                                   // every thread has read the flags
  if (!lead) return;
  const int step = D.ctl[BUNDLE_STEP];
  float *h = D.history + 4 * (size_t)step;
  h[0] = broken ? pose_one_nan(NAN) : pose_one_nan(c2[0]);
  h[1] = lam;
  int *hi = reinterpret_cast<int *>(h);
  hi[2] = kept ? 1 : 0;
  hi[3] = D.ctl[BUNDLE_ITERS];
  if (kept) {
    D.ctl[BUNDLE_CUR] = 1 - D.ctl[BUNDLE_CUR];
    D.ctl[BUNDLE_KEPT] = D.ctl[BUNDLE_KEPT] + 1;
    D.fctl[BUNDLE_COST] = c2[0];
    const float l = lam / 10.0f;
    D.fctl[BUNDLE_LAM] = l > BUNDLE_LAMBDA_FLOOR ? l : BUNDLE_LAMBDA_FLOOR;
  } else {
    D.fctl[BUNDLE_LAM] = lam * 10.0f;
  }
  D.ctl[BUNDLE_STEP] = step + 1;
  D.ctl[BUNDLE_FAIL] = D.ctl[BUNDLE_BAD] = D.ctl[BUNDLE_ALIVE] = D.ctl[BUNDLE_ITERS] = 0;
}

// ---- outputs

FUND_HD float bundle_rms(float cost, int n) { return n > 0 ? pose_one_nan(sqrtf(cost / (float)n)) : pose_one_nan(NAN); }

FUND_HD void bundle_image_out(const BundleData &D, int i)
{
  const int state = D.istate[i], n = D.icount[i];
  const unsigned *given = reinterpret_cast<const unsigned *>(D.s.cam) + 12 * (size_t)i;
  const unsigned *mine = reinterpret_cast<const unsigned *>(D.cams) + 12 * ((size_t)D.ctl[BUNDLE_CUR] * D.s.nimages + i);
  const bool own = state == BUNDLE_ADJUSTED || state == BUNDLE_FEW_OBS;
  unsigned w[12];
#pragma unroll
  for (int j = 0; j < 12; j++) w[j] = own ? mine[j] : given[j];
  unsigned *out = reinterpret_cast<unsigned *>(D.cam_out) + 12 * (size_t)i;
#pragma unroll
  for (int j = 0; j < 12; j++) out[j] = w[j];
  D.cam_obs[i] = n;
  D.cam_status[i] = state;
  D.cam_rms[2 * (size_t)i] = bundle_rms(D.icost[i], n);
  D.cam_rms[2 * (size_t)i + 1] = bundle_rms(D.icost[(size_t)D.s.nimages + i], n);
  bundle_count(&D.summary[state == BUNDLE_ADJUSTED ? 1 : state == BUNDLE_FEW_OBS ? 3 : state == BUNDLE_HELD ? 5 : 7], 1);
  if (n) bundle_count(&D.summary[2], n);
  if (i == 0) {
    D.summary[0] = scene_T(D.s);
    D.summary[6] = D.ctl[BUNDLE_KEPT];
    D.cost[0] = pose_one_nan(D.fctl[BUNDLE_COST0]);
    D.cost[1] = pose_one_nan(D.fctl[BUNDLE_COST]);
  }
}

FUND_HD void bundle_track_out(const BundleData &D, int t)
{
  const int n = D.tcount[t];
  const unsigned *given = reinterpret_cast<const unsigned *>(D.s.points) + 4 * (size_t)t;
  unsigned w[4] = {given[0], given[1], given[2], given[3]};
  if (bundle_active(D, t)) {
    const int b = D.ctl[BUNDLE_CUR];
    const unsigned *mine = reinterpret_cast<const unsigned *>(D.pts) + 3 * ((size_t)b * D.s.max_tracks + t);
    const float *e = D.eterm + (size_t)b * D.s.max_obs;
    float c = 0.0f;
    const int off = D.s.track_offsets[t], end = D.s.track_offsets[t + 1];
    for (int o = off; o < end; o++)
      if (D.owner[o] == t && D.key[o] >= 0) c = c + e[o];
    const float rms = bundle_rms(c, n);
    w[0] = mine[0]; w[1] = mine[1]; w[2] = mine[2];
    __builtin_memcpy(&w[3], &rms, sizeof rms);
    bundle_count(&D.summary[4], 1);
  }
  unsigned *out = reinterpret_cast<unsigned *>(D.points_out) + 4 * (size_t)t;
  out[0] = w[0]; out[1] = w[1]; out[2] = w[2]; out[3] = w[3];
  D.point_obs[t] = n;
}

// d_obs_weight for slot o < O: -1 for a slot that is no member, w of a member under the final state
FUND_HD void bundle_weight_slot(const BundleData &D, int o)
{
  const int k = D.key[o];
  float w = -1.0f;
  if (k >= 0) {
    const int b = D.ctl[BUNDLE_CUR];
    float c[12];
    bundle_load_cam(D.cams + 12 * ((size_t)b * D.s.nimages + k), c);
    const float *P = D.pts + 3 * ((size_t)b * D.s.max_tracks + D.owner[o]);
    const float X[3] = {P[0], P[1], P[2]};
    const TrackObs ob = track_obs_load(D.s.obs + o);
    RefineView v;
    if (refine_view(c, D.s.intrinsics + 4 * (size_t)k, X, ob.xpos, ob.ypos, v))
      w = pose_one_nan(bundle_loss(D.loss, D.loss_scale, D.loss_scale2, v.ru * v.ru + v.rv * v.rv).w);
    else
      w = pose_one_nan(NAN);                   // the final state has every member in front: not reached
  }
  D.obs_weight[o] = w;
}

// ---- the host's side: the Sum as a loop, the phases in the order of the launches

struct BundleHostSum {
  float p[BUNDLE_NORMAL * FUND_SLOTS];
  void fence() {}
  template <int K, class V>
  void sum(int n, V &v, float (&out)[K])
  {
    for (int t = 0; t < FUND_SLOTS; t++) {
      float acc[K];
      fundamental_slot_partial<K>(t, n, v, acc);
      for (int k = 0; k < K; k++) p[k * FUND_SLOTS + t] = acc[k];
    }
    for (int off = FUND_SLOTS / 2; off > 0; off >>= 1)
      for (int t = 0; t < off; t++) fundamental_tree_step<K>(p, t, off);
    for (int k = 0; k < K; k++) out[k] = p[k * FUND_SLOTS];
  }
};
