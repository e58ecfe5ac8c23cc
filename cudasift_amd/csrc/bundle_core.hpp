// bundle_core.hpp — the arithmetic of misift_adjust_bundle_batch, for host and device: every phase of the call as a
// function of one work item (a slot, a track, an image) over a BundleData, a struct of plain pointers.  The kernels
// (kernels_bundle.hip) hand in the call's arguments and temp memory and run one work item per lane or per workgroup; the
// host-only test hook (misift_test_adjust_bundle) hands in host arrays and runs the same functions in loops.  Both go
// through the phase types at the end of this file, in the order bundle_schedule (bundle_host.hpp) states once for the
// two.  So what a CPU test pins is what the device runs: arithmetic, sequence and instance.  The definition, step by
// step, is in include/misift.h.
// misift_adjust_bundle_robust_batch is the same call with a loss: bundle_loss gives rho, w and
// sqrt(w) of a member's squared residual, step 1 scales the member's 20 values by sqrt(w) where it writes them, the cost
// pass stores rho in place of the squared residual, and every phase downstream reads what those two wrote.  ROBUST is a
// template argument of the two, so the plain call compiles to what it was.  misift_adjust_bundle_focal_batch adds one
// focal scale per camera group: FOCAL is a template argument (or a function of its own, *_focal) of every phase that
// reads the scale, the focal Jacobian of a slot lives in an array of its own beside the 20 values, and the groups'
// scalars are carried by the scalar workgroup beside the images' 6-vectors.  misift_adjust_bundle_radial_batch adds one
// radial coefficient per group, applied to the observation (bundle_radial_apply, which misift_undistort_obs_batch shares):
// RADIAL is a second template argument (or a function of its own, *_radial) of the phases that read an observation or
// carry a scalar; the column of k_g lives in an array of its own beside the focal one.  Every instance without RADIAL
// compiles to what it was.
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
constexpr int BUNDLE_MAX_GROUPS = 8;           // MISIFT_MAX_FOCAL_GROUPS
constexpr int BUNDLE_IMAGE_FOCAL = 9;          // per image with a group: U_cf (6), Uff, gf, the sum of wf . y_t
constexpr int BUNDLE_NORMAL_FOCAL = BUNDLE_NORMAL + BUNDLE_IMAGE_FOCAL;
enum { BUNDLE_FOCAL_REFINED = 0, BUNDLE_FOCAL_NO_MEMBER = 1, BUNDLE_FOCAL_NOT_REFINED = 2 };   // MISIFT_FOCAL_*
constexpr int BUNDLE_IMAGE_RADIAL = 10;        // per image of a radial group: U_ck (6), Ukk, gk, the sum of wk . y_t, Ufk
constexpr int BUNDLE_NORMAL_RADIAL = BUNDLE_NORMAL_FOCAL + BUNDLE_IMAGE_RADIAL;
enum { BUNDLE_RADIAL_REFINED = 0, BUNDLE_RADIAL_NO_MEMBER = 1, BUNDLE_RADIAL_NOT_REFINED = 2,
       BUNDLE_RADIAL_HELD = 3 };               // MISIFT_RADIAL_*

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
  // misift_adjust_bundle_focal_batch only (the FOCAL instances): one focal scale per camera group
  int ngroups;
  const int *grp;                              // nimages: the group of the image, or -1
  int *fcount;                                 // BUNDLE_MAX_GROUPS: the members in the group's images
  float *fs;                                   // 2 x BUNDLE_MAX_GROUPS: s_g in the two state buffers
  float *fvec;                                 // 5 x BUNDLE_MAX_GROUPS: x, r, z, p, y of the groups
  float *fsc;                                  // 2 x BUNDLE_MAX_GROUPS: l1 * U_gg, then S_gg
  float *flin;                                 // max_obs x 2: Juf, Jvf of a slot
  float *tfd;                                  // max_tracks x BUNDLE_MAX_GROUPS: w_gt . SOLVE(V'_t, w_gt)
  float *iuf;                                  // nimages x BUNDLE_IMAGE_FOCAL: U_cf (6), then the sums of Uff, gf, wf . y_t
  float *ifv;                                  // nimages x 2 per CG iteration: U_cf . p_i, the sum of wf . q_t
  float *intrinsics_out;                       // nimages x 4
  int *focal_out;                              // ngroups x 3 words: s_g, the members, the status
  // misift_adjust_bundle_radial_batch only (the RADIAL instances): one radial coefficient per camera group
  const int *rad;                              // BUNDLE_MAX_GROUPS flags: k_g is an unknown (0 from ngroups on)
  const float *k0;                             // BUNDLE_MAX_GROUPS: k_g at the start (0 from ngroups on)
  float *ks;                                   // 2 x BUNDLE_MAX_GROUPS: k_g in the two state buffers
  float *kvec;                                 // 5 x BUNDLE_MAX_GROUPS: x, r, z, p, y of the coefficients
  float *ksc;                                  // 3 x BUNDLE_MAX_GROUPS: l1 * U_kk, then S_kk, then U_fk
  float *rlin;                                 // max_obs x 2: Juk, Jvk of a slot
  float *tkd;                                  // max_tracks x BUNDLE_MAX_GROUPS: wk_gt . SOLVE(V'_t, wk_gt)
  float *iuk;                                  // nimages x BUNDLE_IMAGE_RADIAL: U_ck (6), then the sums of Ukk, gk, wk . y_t, Ufk
  float *ikv;                                  // nimages x 2 per CG iteration: U_ck . p_i, the sum of wk . q_t
  int *radial_out;                             // ngroups x 3 words: k_g, the members, the status
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

// The radial model of include/misift.h, on an observation: every operation rounded on its own.  k = the given fx fy cx cy
FUND_HD void bundle_radial_apply(const float *k, float coef, float &x, float &y, float &qu, float &qv)
{
  const float dx = x - k[2], dy = y - k[3];
  const float nx = dx / k[0], ny = dy / k[1];
  const float rho2 = nx * nx + ny * ny;
  const float e = coef * rho2;
  qu = dx * rho2;
  qv = dy * rho2;
  x = x + dx * e;
  y = y + dy * e;
}
// RADIAL: the observation of slot o in image k as it enters under the coefficients `ks` (one per group); otherwise, and
// for an image without a group, as given
template <bool RADIAL>
FUND_HD void bundle_observe(const BundleData &D, const float *ks, int k, const TrackObs &ob, float &x, float &y)
{
  x = ob.xpos;
  y = ob.ypos;
  if (!RADIAL) return;
  const int g = D.grp[k];
  if (g < 0) return;
  float qu, qv;
  bundle_radial_apply(D.s.intrinsics + 4 * (size_t)k, ks[g], x, y, qu, qv);
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

// slot o < O: a candidate stays in `key` iff it is a pre-member (RADIAL: of the observation under k0)
template <bool RADIAL = false>
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
    float x, y;
    bundle_observe<RADIAL>(D, D.k0, k, ob, x, y);
    in = refine_member(c, D.s.intrinsics + 4 * (size_t)k, X, x, y, D.thresh2);
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

// FOCAL: the intrinsics a member of image k is projected with under state buffer b: fx*s_g, fy*s_g, cx, cy, each
// product rounded (s = 1 for an image without a group); otherwise the intrinsics as given
template <bool FOCAL>
FUND_HD const float *bundle_intrinsics(const BundleData &D, int b, int k, float (&kk)[4])
{
  const float *given = D.s.intrinsics + 4 * (size_t)k;
  if (!FOCAL) return given;
  const int g = D.grp[k];
  const float s = g >= 0 ? D.fs[b * BUNDLE_MAX_GROUPS + g] : 1.0f;
  kk[0] = given[0] * s; kk[1] = given[1] * s; kk[2] = given[2]; kk[3] = given[3];
  return kk;
}
// wf[q] = Juf*Pu[q] + Jvf*Pv[q] of slot o, and wf . v
FUND_HD float bundle_wf(const float *l, const float *f, int q) { return f[0] * l[12 + q] + f[1] * l[15 + q]; }
FUND_HD float bundle_wf3(const float *l, const float *f, const float *v)
{
  return (bundle_wf(l, f, 0) * v[0] + bundle_wf(l, f, 1) * v[1]) + bundle_wf(l, f, 2) * v[2];
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
template <bool ROBUST, bool FOCAL = false, bool RADIAL = false>
FUND_HD void bundle_eval_slot(const BundleData &D, int o, bool trial)
{
  const int k = D.key[o];
  if (k < 0) return;
  if (trial && D.ctl[BUNDLE_FAIL]) return;
  const int b = trial ? 1 - D.ctl[BUNDLE_CUR] : D.ctl[BUNDLE_CUR];
  float c[12], kk[4];
  bundle_load_cam(D.cams + 12 * ((size_t)b * D.s.nimages + k), c);
  const float *P = D.pts + 3 * ((size_t)b * D.s.max_tracks + D.owner[o]);
  const float X[3] = {P[0], P[1], P[2]};
  const TrackObs ob = track_obs_load(D.s.obs + o);
  RefineView v;
  float e = 0.0f, x, y;
  bundle_observe<RADIAL>(D, D.ks + b * BUNDLE_MAX_GROUPS, k, ob, x, y);
  if (refine_view(c, bundle_intrinsics<FOCAL>(D, b, k, kk), X, x, y, v)) {
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

// FOCAL, in the scalar workgroup before any state is evaluated: s_g = 1 in both buffers, the members of every group
// RADIAL: and k_g = k0_g in both buffers
template <bool RADIAL = false, class Sum>
FUND_HD void bundle_focal_init(const BundleData &D, Sum &S, int lane, int lanes)
{
  for (int g = lane; g < BUNDLE_MAX_GROUPS; g += lanes) {
    D.fcount[g] = 0;
    D.fs[g] = D.fs[BUNDLE_MAX_GROUPS + g] = 1.0f;
    if (RADIAL) D.ks[g] = D.ks[BUNDLE_MAX_GROUPS + g] = D.k0[g];
  }
  S.fence();
  for (int i = lane; i < D.s.nimages; i += lanes) {
    const int g = D.grp[i];
    if (g >= 0 && D.icount[i] > 0) bundle_count(&D.fcount[g], D.icount[i]);
  }
  S.fence();
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

// FOCAL: the groups' vector `which`; a group is live iff an image of it has a member
FUND_HD float *bundle_fvec(const BundleData &D, int which) { return D.fvec + which * BUNDLE_MAX_GROUPS; }
FUND_HD bool bundle_group_live(const BundleData &D, int g) { return D.fcount[g] > 0; }
// RADIAL: a coefficient is live iff it is an unknown and its group is live; wk[q] = Juk*Pu[q] + Jvk*Pv[q] of slot o
FUND_HD bool bundle_radial_live(const BundleData &D, int g) { return D.rad[g] != 0 && D.fcount[g] > 0; }
FUND_HD float bundle_wk(const float *l, const float *f, int q) { return f[0] * l[12 + q] + f[1] * l[15 + q]; }
FUND_HD float bundle_wk3(const float *l, const float *f, const float *v)
{
  return (bundle_wk(l, f, 0) * v[0] + bundle_wk(l, f, 1) * v[1]) + bundle_wk(l, f, 2) * v[2];
}

// FOCAL: bundle_track_normal with the focal Jacobian of every member beside the 20 values (Juf = fx*a, Jvf = fy*b with
// the given fx, fy, times sw under a loss), and per group w_gt . SOLVE(V', w_gt) for the group's Schur scalar.  A function
// of its own, so that the plain one compiles to what it was.  RADIAL: the observation enters as (x', y') under k_g of the
// state; a member of a group whose k_g is an unknown has the column Juk = -(dx*rho2), Jvk = -(dy*rho2) (ru = x' - u
// grows by dx*rho2 per unit of k, so the column has the sign of the others: r falls by J times the step), times sw
// under a loss, any other member zeros; per group wk_gt . V'^-1 wk_gt from one more walk that reuses the registers of w_gt
template <bool ROBUST, bool RADIAL = false>
FUND_HD void bundle_track_normal_focal(const BundleData &D, int t)
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
    float c[12], l[BUNDLE_LIN], kk[4], f[2];
    bundle_load_cam(D.cams + 12 * ((size_t)b * D.s.nimages + k), c);
    const TrackObs ob = track_obs_load(D.s.obs + o);
    const float *kp = bundle_intrinsics<true>(D, b, k, kk);
    float x = ob.xpos, y = ob.ypos, rk[2] = {0.0f, 0.0f};
    if (RADIAL) {
      const int g = D.grp[k];
      if (g >= 0) {
        float qu, qv;
        bundle_radial_apply(D.s.intrinsics + 4 * (size_t)k, D.ks[b * BUNDLE_MAX_GROUPS + g], x, y, qu, qv);
        if (D.rad[g]) {
          rk[0] = -qu;
          rk[1] = -qv;
        }
      }
    }
    if (!bundle_linearise(c, kp, X, x, y, l)) {
      bundle_raise(&D.ctl[BUNDLE_FAIL]);       // the state has every member in front: not reached
#pragma unroll
      for (int j = 0; j < BUNDLE_LIN; j++) l[j] = 0.0f;
    }
    RefineView view;                           // a, b of the same view once more: the same bits
    const bool front = refine_view(c, kp, X, x, y, view);
    f[0] = front ? D.s.intrinsics[4 * (size_t)k] * view.a : 0.0f;
    f[1] = front ? D.s.intrinsics[4 * (size_t)k + 1] * view.b : 0.0f;
    if (ROBUST) {
      const float sw = bundle_loss(D.loss, D.loss_scale, D.loss_scale2, l[18] * l[18] + l[19] * l[19]).sw;
#pragma unroll
      for (int j = 0; j < BUNDLE_LIN; j++) l[j] = sw * l[j];
      f[0] = sw * f[0];
      f[1] = sw * f[1];
      if (RADIAL) {
        rk[0] = sw * rk[0];
        rk[1] = sw * rk[1];
      }
    }
    float *dst = D.lin + (size_t)BUNDLE_LIN * o;
#pragma unroll
    for (int j = 0; j < BUNDLE_LIN; j++) dst[j] = l[j];
    D.flin[2 * (size_t)o] = f[0];
    D.flin[2 * (size_t)o + 1] = f[1];
    if (RADIAL) {
      D.rlin[2 * (size_t)o] = rk[0];
      D.rlin[2 * (size_t)o + 1] = rk[1];
    }
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
  // w_gt of every group in one more walk over the members: BUNDLE_MAX_GROUPS 3-vectors, every index a constant of the
  // unrolled loop so that they stay in registers; a member adds to its own group's alone
  float w[BUNDLE_MAX_GROUPS][3];
#pragma unroll
  for (int g = 0; g < BUNDLE_MAX_GROUPS; g++) w[g][0] = w[g][1] = w[g][2] = 0.0f;
  for (int o = off; o < end; o++) {
    const int k = D.key[o];
    if (D.owner[o] != t || k < 0) continue;
    const int mine = D.grp[k];
    if (mine < 0) continue;
    const float *l = D.lin + (size_t)BUNDLE_LIN * o, *f = D.flin + 2 * (size_t)o;
    const float wf[3] = {bundle_wf(l, f, 0), bundle_wf(l, f, 1), bundle_wf(l, f, 2)};
#pragma unroll
    for (int g = 0; g < BUNDLE_MAX_GROUPS; g++)
#pragma unroll
      for (int j = 0; j < 3; j++) w[g][j] = mine == g ? w[g][j] + wf[j] : w[g][j];
  }
#pragma unroll
  for (int g = 0; g < BUNDLE_MAX_GROUPS; g++) {
    if (g >= D.ngroups || !bundle_group_live(D, g)) continue;
    float x[3];
    N.g0 = w[g][0]; N.g1 = w[g][1]; N.g2 = w[g][2];
    tri_solve(N, x);                           // a failed solve gives zeros, and has failed the step above
    D.tfd[(size_t)BUNDLE_MAX_GROUPS * t + g] = (w[g][0] * x[0] + w[g][1] * x[1]) + w[g][2] * x[2];
  }
  if (!RADIAL) return;
  // wk_gt in the same registers: the members of the groups whose k_g is an unknown
#pragma unroll
  for (int g = 0; g < BUNDLE_MAX_GROUPS; g++) w[g][0] = w[g][1] = w[g][2] = 0.0f;
  for (int o = off; o < end; o++) {
    const int k = D.key[o];
    if (D.owner[o] != t || k < 0) continue;
    const int mine = D.grp[k];
    if (mine < 0 || !D.rad[mine]) continue;
    const float *l = D.lin + (size_t)BUNDLE_LIN * o, *f = D.rlin + 2 * (size_t)o;
    const float wk[3] = {bundle_wk(l, f, 0), bundle_wk(l, f, 1), bundle_wk(l, f, 2)};
#pragma unroll
    for (int g = 0; g < BUNDLE_MAX_GROUPS; g++)
#pragma unroll
      for (int j = 0; j < 3; j++) w[g][j] = mine == g ? w[g][j] + wk[j] : w[g][j];
  }
#pragma unroll
  for (int g = 0; g < BUNDLE_MAX_GROUPS; g++) {
    if (g >= D.ngroups || !bundle_radial_live(D, g)) continue;
    float x[3];
    N.g0 = w[g][0]; N.g1 = w[g][1]; N.g2 = w[g][2];
    tri_solve(N, x);
    D.tkd[(size_t)BUNDLE_MAX_GROUPS * t + g] = (w[g][0] * x[0] + w[g][1] * x[1]) + w[g][2] * x[2];
  }
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
// FOCAL: a member in an image of group g then adds wf * v_g, whatever the image's status
// RADIAL: and then wk * v_k when k_g is an unknown
template <bool FOCAL = false, bool RADIAL = false>
FUND_HD void bundle_track_gather(const BundleData &D, int t, int which, float (&s)[3])
{
  s[0] = s[1] = s[2] = 0.0f;
  const int off = D.s.track_offsets[t], end = D.s.track_offsets[t + 1];
  for (int o = off; o < end; o++) {
    const int k = D.key[o];
    if (D.owner[o] != t || k < 0) continue;
    const float *l = D.lin + (size_t)BUNDLE_LIN * o;
    if (D.istate[k] == BUNDLE_ADJUSTED) {
      const float *v = bundle_vec(D, which, k);
#pragma unroll
      for (int q = 0; q < 3; q++) s[q] = s[q] + bundle_wt6(l, q, v);
    }
    if (FOCAL) {
      const int g = D.grp[k];
      if (g < 0) continue;
      const float *f = D.flin + 2 * (size_t)o;
      const float vg = D.fvec[which * BUNDLE_MAX_GROUPS + g];
#pragma unroll
      for (int q = 0; q < 3; q++) s[q] = s[q] + bundle_wf(l, f, q) * vg;
      if (RADIAL && D.rad[g]) {
        const float *rk = D.rlin + 2 * (size_t)o;
        const float vk = D.kvec[which * BUNDLE_MAX_GROUPS + g];
#pragma unroll
        for (int q = 0; q < 3; q++) s[q] = s[q] + bundle_wk(l, rk, q) * vk;
      }
    }
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
// FOCAL: the three focal sums of an image with a group (Uff, gf, wf . y_t), after the 33 and U_cf when it is free
struct BundleFocalTerm {
  const BundleData &D;
  const int *list;
  FUND_HD void focal(int o, float *x) const
  {
    const float *l = D.lin + (size_t)BUNDLE_LIN * o, *f = D.flin + 2 * (size_t)o, *y = D.tq + 3 * (size_t)D.owner[o];
    x[0] = f[0] * f[0] + f[1] * f[1];
    x[1] = f[0] * l[18] + f[1] * l[19];
    x[2] = bundle_wf3(l, f, y);
  }
  FUND_HD bool operator()(int p, float (&x)[3]) const
  {
    focal(list[p], x);
    return true;
  }
  // the 42 values of a free image with a group into x[0 .. 41]
  FUND_HD void all(int p, float *x) const
  {
    const int o = list[p];
    BundleNormalTerm base{D, list};
    base(p, *reinterpret_cast<float(*)[BUNDLE_NORMAL]>(x));
    const float *l = D.lin + (size_t)BUNDLE_LIN * o, *f = D.flin + 2 * (size_t)o;
#pragma unroll
    for (int r = 0; r < 6; r++) x[BUNDLE_NORMAL + r] = l[r] * f[0] + l[6 + r] * f[1];
    focal(o, x + BUNDLE_NORMAL + 6);
  }
  FUND_HD bool operator()(int p, float (&x)[BUNDLE_NORMAL_FOCAL]) const
  {
    all(p, x);
    return true;
  }
};
// the lead thread's half of step 3: U', b from the 33 sums, the LDL^T checked
FUND_HD void bundle_image_normal_finish(const BundleData &D, int i, const float *s)
{
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
template <class Sum>
FUND_HD void bundle_image_normal(const BundleData &D, Sum &S, int i, bool lead)
{
  if (D.istate[i] != BUNDLE_ADJUSTED) return;
  BundleNormalTerm term{D, D.list + D.istart[i]};
  float s[BUNDLE_NORMAL];
  S.template sum<BUNDLE_NORMAL>(D.icount[i], term, s);
  if (lead) bundle_image_normal_finish(D, i, s);
}
// FOCAL: a usable image with a group takes the three focal sums too, a free one among them the six of U_cf: 42 sums
template <class Sum>
FUND_HD void bundle_image_normal_focal(const BundleData &D, Sum &S, int i, bool lead)
{
  if (D.grp[i] < 0) return bundle_image_normal(D, S, i, lead);
  if (D.istate[i] == BUNDLE_NO_CAMERA) return;
  BundleFocalTerm term{D, D.list + D.istart[i]};
  float *dst = D.iuf + (size_t)BUNDLE_IMAGE_FOCAL * i;
  if (D.istate[i] != BUNDLE_ADJUSTED) {
    float s[3];
    S.template sum<3>(D.icount[i], term, s);
    if (!lead) return;
#pragma unroll
    for (int r = 0; r < 6; r++) dst[r] = 0.0f;
    dst[6] = s[0]; dst[7] = s[1]; dst[8] = s[2];
    return;
  }
  float s[BUNDLE_NORMAL_FOCAL];
  S.template sum<BUNDLE_NORMAL_FOCAL>(D.icount[i], term, s);
  if (!lead) return;
#pragma unroll
  for (int r = 0; r < BUNDLE_IMAGE_FOCAL; r++) dst[r] = s[BUNDLE_NORMAL + r];
  bundle_image_normal_finish(D, i, s);
}

// RADIAL: a usable image of a group whose k_g is an unknown takes four more sums (Ukk, gk, wk . y_t, Ufk), a free one
// among them the six of U_ck: 52 sums.  Any other image is the focal call's
struct BundleRadialTerm {
  const BundleData &D;
  const int *list;
  FUND_HD void radial(int o, float *x) const
  {
    const float *l = D.lin + (size_t)BUNDLE_LIN * o, *f = D.flin + 2 * (size_t)o, *k = D.rlin + 2 * (size_t)o;
    const float *y = D.tq + 3 * (size_t)D.owner[o];
    x[0] = k[0] * k[0] + k[1] * k[1];
    x[1] = k[0] * l[18] + k[1] * l[19];
    x[2] = bundle_wk3(l, k, y);
    x[3] = f[0] * k[0] + f[1] * k[1];
  }
  FUND_HD bool operator()(int p, float (&x)[7]) const
  {
    BundleFocalTerm base{D, list};
    base.focal(list[p], x);
    radial(list[p], x + 3);
    return true;
  }
  FUND_HD bool operator()(int p, float (&x)[BUNDLE_NORMAL_RADIAL]) const
  {
    const int o = list[p];
    BundleFocalTerm base{D, list};
    base.all(p, x);
    const float *l = D.lin + (size_t)BUNDLE_LIN * o, *k = D.rlin + 2 * (size_t)o;
#pragma unroll
    for (int r = 0; r < 6; r++) x[BUNDLE_NORMAL_FOCAL + r] = l[r] * k[0] + l[6 + r] * k[1];
    radial(o, x + BUNDLE_NORMAL_FOCAL + 6);
    return true;
  }
};
template <class Sum>
FUND_HD void bundle_image_normal_radial(const BundleData &D, Sum &S, int i, bool lead)
{
  const int g = D.grp[i];
  if (g < 0 || !D.rad[g]) return bundle_image_normal_focal(D, S, i, lead);
  if (D.istate[i] == BUNDLE_NO_CAMERA) return;
  BundleRadialTerm term{D, D.list + D.istart[i]};
  float *dst = D.iuf + (size_t)BUNDLE_IMAGE_FOCAL * i, *dk = D.iuk + (size_t)BUNDLE_IMAGE_RADIAL * i;
  if (D.istate[i] != BUNDLE_ADJUSTED) {
    float s[7];
    S.template sum<7>(D.icount[i], term, s);
    if (!lead) return;
#pragma unroll
    for (int r = 0; r < 6; r++) dst[r] = dk[r] = 0.0f;
    dst[6] = s[0]; dst[7] = s[1]; dst[8] = s[2];
    dk[6] = s[3]; dk[7] = s[4]; dk[8] = s[5]; dk[9] = s[6];
    return;
  }
  float s[BUNDLE_NORMAL_RADIAL];
  S.template sum<BUNDLE_NORMAL_RADIAL>(D.icount[i], term, s);
  if (!lead) return;
#pragma unroll
  for (int r = 0; r < BUNDLE_IMAGE_FOCAL; r++) dst[r] = s[BUNDLE_NORMAL + r];
#pragma unroll
  for (int r = 0; r < BUNDLE_IMAGE_RADIAL; r++) dk[r] = s[BUNDLE_NORMAL_FOCAL + r];
  bundle_image_normal_finish(D, i, s);
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

// FOCAL: the cross-image and cross-track sums of group g, and the groups' share of a dot product (ascending live g)
struct BundleGroupNormalTerm {
  const BundleData &D;
  int g;
  FUND_HD bool operator()(int i, float (&x)[3]) const
  {
    if (D.grp[i] != g || D.istate[i] == BUNDLE_NO_CAMERA) return false;
    const float *src = D.iuf + (size_t)BUNDLE_IMAGE_FOCAL * i + 6;
    x[0] = src[0]; x[1] = src[1]; x[2] = src[2];
    return true;
  }
};
struct BundleGroupCgTerm {
  const BundleData &D;
  int g;
  FUND_HD bool operator()(int i, float (&x)[2]) const
  {
    if (D.grp[i] != g || D.istate[i] == BUNDLE_NO_CAMERA) return false;
    x[0] = D.ifv[2 * (size_t)i]; x[1] = D.ifv[2 * (size_t)i + 1];
    return true;
  }
};
struct BundleGroupSchurTerm {
  const BundleData &D;
  int g;
  FUND_HD bool operator()(int t, float (&x)[1]) const
  {
    if (!(D.tcount[t] >= D.min_views)) return false;
    x[0] = D.tfd[(size_t)BUNDLE_MAX_GROUPS * t + g];
    return true;
  }
};
// RADIAL: the same three for the coefficient of group g, and its share of a dot product behind the focal scalars'
struct BundleGroupRadialTerm {
  const BundleData &D;
  int g;
  FUND_HD bool operator()(int i, float (&x)[4]) const
  {
    if (D.grp[i] != g || D.istate[i] == BUNDLE_NO_CAMERA) return false;
    const float *src = D.iuk + (size_t)BUNDLE_IMAGE_RADIAL * i + 6;
    x[0] = src[0]; x[1] = src[1]; x[2] = src[2]; x[3] = src[3];
    return true;
  }
};
struct BundleGroupCgRadialTerm {
  const BundleData &D;
  int g;
  FUND_HD bool operator()(int i, float (&x)[2]) const
  {
    if (D.grp[i] != g || D.istate[i] == BUNDLE_NO_CAMERA) return false;
    x[0] = D.ikv[2 * (size_t)i]; x[1] = D.ikv[2 * (size_t)i + 1];
    return true;
  }
};
struct BundleGroupSchurRadialTerm {
  const BundleData &D;
  int g;
  FUND_HD bool operator()(int t, float (&x)[1]) const
  {
    if (!(D.tcount[t] >= D.min_views)) return false;
    x[0] = D.tkd[(size_t)BUNDLE_MAX_GROUPS * t + g];
    return true;
  }
};
FUND_HD float *bundle_kvec(const BundleData &D, int which) { return D.kvec + which * BUNDLE_MAX_GROUPS; }
template <bool FOCAL, bool RADIAL = false>
FUND_HD float bundle_dot_groups(const BundleData &D, float acc, int a, int b)
{
  if (FOCAL)
    for (int g = 0; g < D.ngroups; g++)
      if (bundle_group_live(D, g)) acc = acc + bundle_fvec(D, a)[g] * bundle_fvec(D, b)[g];
  if (RADIAL)
    for (int g = 0; g < D.ngroups; g++)
      if (bundle_radial_live(D, g)) acc = acc + bundle_kvec(D, a)[g] * bundle_kvec(D, b)[g];
  return acc;
}

// step 4, the start of PCG in the scalar workgroup; this thread takes the images lane, lane + lanes, ...
// FOCAL: per live group U_gg, g_g, the Schur scalar S_gg (not finite and > 0: the step fails), x, r, z = r / S_gg, p
// RADIAL: then per group with a live coefficient U_kk, g_k, U_fk and the Schur scalar S_kk in the same way
template <bool FOCAL = false, bool RADIAL = false, class Sum>
FUND_HD void bundle_cg_start(const BundleData &D, Sum &S, int lane, int lanes, bool lead)
{
  bool fail = D.ctl[BUNDLE_FAIL] != 0;
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
  if (FOCAL && !fail) {
    const float lam1 = 1.0f + D.fctl[BUNDLE_LAM];
    const int T = scene_T(D.s);
    for (int g = 0; g < D.ngroups; g++) {
      if (!bundle_group_live(D, g)) continue;
      BundleGroupNormalTerm nterm{D, g};
      BundleGroupSchurTerm sterm{D, g};
      float u[3], d[1];
      S.template sum<3>(D.s.nimages, nterm, u);
      S.template sum<1>(T, sterm, d);
      const float ul = u[0] * lam1, sg = ul - d[0], bg = u[1] - u[2];
      if (!(fundamental_finite(sg) && sg > 0.0f)) fail = true;
      if (!lead) continue;
      D.fsc[g] = ul;
      D.fsc[BUNDLE_MAX_GROUPS + g] = sg;
      bundle_fvec(D, BUNDLE_X)[g] = 0.0f;
      bundle_fvec(D, BUNDLE_R)[g] = bg;
      bundle_fvec(D, BUNDLE_Z)[g] = bundle_fvec(D, BUNDLE_P)[g] = bg / sg;
    }
    if (RADIAL)
      for (int g = 0; g < D.ngroups; g++) {
        if (!bundle_radial_live(D, g)) continue;
        BundleGroupRadialTerm nterm{D, g};
        BundleGroupSchurRadialTerm sterm{D, g};
        float u[4], d[1];
        S.template sum<4>(D.s.nimages, nterm, u);
        S.template sum<1>(T, sterm, d);
        const float ul = u[0] * lam1, sk = ul - d[0], bk = u[1] - u[2];
        if (!(fundamental_finite(sk) && sk > 0.0f)) fail = true;
        if (!lead) continue;
        D.ksc[g] = ul;
        D.ksc[BUNDLE_MAX_GROUPS + g] = sk;
        D.ksc[2 * BUNDLE_MAX_GROUPS + g] = u[3];
        bundle_kvec(D, BUNDLE_X)[g] = 0.0f;
        bundle_kvec(D, BUNDLE_R)[g] = bk;
        bundle_kvec(D, BUNDLE_Z)[g] = bundle_kvec(D, BUNDLE_P)[g] = bk / sk;
      }
    if (fail && lead) bundle_raise(&D.ctl[BUNDLE_FAIL]);
  }
  float rho[1] = {0.0f};
  if (!fail) {                                 // the same in every thread
    S.fence();
    BundleDotTerm term{D.istate, D.ivec + 6 * (size_t)BUNDLE_R * D.s.nimages, D.ivec + 6 * (size_t)BUNDLE_Z * D.s.nimages};
    S.template sum<1>(D.s.nimages, term, rho);
    rho[0] = bundle_dot_groups<FOCAL, RADIAL>(D, rho[0], BUNDLE_R, BUNDLE_Z);
  }
  if (!lead) return;
  D.fctl[BUNDLE_RHO] = rho[0];
  D.ctl[BUNDLE_ALIVE] = (!fail && fundamental_finite(rho[0])) ? 1 : 0;
  D.ctl[BUNDLE_ITERS] = 0;
}

// a CG iteration, per active track: q_t = V'^-1 sum W^T p_image
template <bool FOCAL = false, bool RADIAL = false>
FUND_HD void bundle_cg_track(const BundleData &D, int t)
{
  if (!D.ctl[BUNDLE_ALIVE] || !bundle_active(D, t)) return;
  float s[3], q[3];
  bundle_track_gather<FOCAL, RADIAL>(D, t, BUNDLE_P, s);
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
// FOCAL: a usable image with a group sums wf . q_t too; a free one has y_i[r] = (U'[r] . p_i + U_cf[r]*p_g) - ...
struct BundleWqFocalTerm {
  const BundleData &D;
  const int *list;
  FUND_HD bool operator()(int p, float (&x)[1]) const
  {
    const int o = list[p];
    x[0] = bundle_wf3(D.lin + (size_t)BUNDLE_LIN * o, D.flin + 2 * (size_t)o, D.tq + 3 * (size_t)D.owner[o]);
    return true;
  }
  FUND_HD bool operator()(int p, float (&x)[7]) const
  {
    const int o = list[p];
    const float *l = D.lin + (size_t)BUNDLE_LIN * o, *q = D.tq + 3 * (size_t)D.owner[o];
#pragma unroll
    for (int r = 0; r < 6; r++) x[r] = bundle_w3(l, r, q);
    x[6] = bundle_wf3(l, D.flin + 2 * (size_t)o, q);
    return true;
  }
};
template <class Sum>
FUND_HD void bundle_cg_image_focal(const BundleData &D, Sum &S, int i, bool lead)
{
  const int g = D.grp[i];
  if (g < 0) return bundle_cg_image(D, S, i, lead);
  if (!D.ctl[BUNDLE_ALIVE] || D.istate[i] == BUNDLE_NO_CAMERA) return;
  BundleWqFocalTerm term{D, D.list + D.istart[i]};
  float *dst = D.ifv + 2 * (size_t)i;
  if (D.istate[i] != BUNDLE_ADJUSTED) {
    float s[1];
    S.template sum<1>(D.icount[i], term, s);
    if (!lead) return;
    dst[0] = 0.0f;
    dst[1] = s[0];
    return;
  }
  float s[7];
  S.template sum<7>(D.icount[i], term, s);
  if (!lead) return;
  const float *src = D.iu + (size_t)REFINE_SUMS * i, *p = bundle_vec(D, BUNDLE_P, i);
  const float *ucf = D.iuf + (size_t)BUNDLE_IMAGE_FOCAL * i;
  const float pg = bundle_fvec(D, BUNDLE_P)[g];
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
  for (int r = 0; r < 6; r++) y[r] = (bundle_dot6(U[r], p) + ucf[r] * pg) - s[r];
  dst[0] = bundle_dot6(ucf, p);
  dst[1] = s[6];
}

// RADIAL: a usable image of a group whose k_g is an unknown sums wk . q_t too; a free one has
// y_i[r] = ((U'[r] . p_i + U_cf[r]*p_g) + U_ck[r]*p_k) - ...  Any other image is the focal call's
struct BundleWqRadialTerm {
  const BundleData &D;
  const int *list;
  FUND_HD bool operator()(int p, float (&x)[2]) const
  {
    const int o = list[p];
    const float *l = D.lin + (size_t)BUNDLE_LIN * o, *q = D.tq + 3 * (size_t)D.owner[o];
    x[0] = bundle_wf3(l, D.flin + 2 * (size_t)o, q);
    x[1] = bundle_wk3(l, D.rlin + 2 * (size_t)o, q);
    return true;
  }
  FUND_HD bool operator()(int p, float (&x)[8]) const
  {
    const int o = list[p];
    const float *l = D.lin + (size_t)BUNDLE_LIN * o, *q = D.tq + 3 * (size_t)D.owner[o];
#pragma unroll
    for (int r = 0; r < 6; r++) x[r] = bundle_w3(l, r, q);
    x[6] = bundle_wf3(l, D.flin + 2 * (size_t)o, q);
    x[7] = bundle_wk3(l, D.rlin + 2 * (size_t)o, q);
    return true;
  }
};
template <class Sum>
FUND_HD void bundle_cg_image_radial(const BundleData &D, Sum &S, int i, bool lead)
{
  const int g = D.grp[i];
  if (g < 0 || !D.rad[g]) return bundle_cg_image_focal(D, S, i, lead);
  if (!D.ctl[BUNDLE_ALIVE] || D.istate[i] == BUNDLE_NO_CAMERA) return;
  BundleWqRadialTerm term{D, D.list + D.istart[i]};
  float *dst = D.ifv + 2 * (size_t)i, *dk = D.ikv + 2 * (size_t)i;
  if (D.istate[i] != BUNDLE_ADJUSTED) {
    float s[2];
    S.template sum<2>(D.icount[i], term, s);
    if (!lead) return;
    dst[0] = dk[0] = 0.0f;
    dst[1] = s[0];
    dk[1] = s[1];
    return;
  }
  float s[8];
  S.template sum<8>(D.icount[i], term, s);
  if (!lead) return;
  const float *src = D.iu + (size_t)REFINE_SUMS * i, *p = bundle_vec(D, BUNDLE_P, i);
  const float *ucf = D.iuf + (size_t)BUNDLE_IMAGE_FOCAL * i, *uck = D.iuk + (size_t)BUNDLE_IMAGE_RADIAL * i;
  const float pg = bundle_fvec(D, BUNDLE_P)[g], pk = bundle_kvec(D, BUNDLE_P)[g];
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
  for (int r = 0; r < 6; r++) y[r] = ((bundle_dot6(U[r], p) + ucf[r] * pg) + uck[r] * pk) - s[r];
  dst[0] = bundle_dot6(ucf, p);
  dst[1] = s[6];
  dk[0] = bundle_dot6(uck, p);
  dk[1] = s[7];
}

// a CG iteration in the scalar workgroup: sigma, alpha, x, r, z, rho', beta, p
// FOCAL: first y_g = (l1*U_gg * p_g + the cross-image sum of U_cf . p_i) - the cross-image sum of the sums of wf . q_t
// RADIAL: a group with a live coefficient has y_g = ((l1*U_gg * p_g + U_fk * p_k) + ...) - ..., and
// y_k = ((l1*U_kk * p_k + U_fk * p_g) + the cross-image sum of U_ck . p_i) - the cross-image sum of the sums of wk . q_t
template <bool FOCAL = false, bool RADIAL = false, class Sum>
FUND_HD void bundle_cg_scalar(const BundleData &D, Sum &S, int lane, int lanes, bool lead)
{
  if (!D.ctl[BUNDLE_ALIVE]) return;            // the same in every thread
  const float rho = D.fctl[BUNDLE_RHO];
  const size_t n6 = 6 * (size_t)D.s.nimages;
  if (FOCAL) {
    for (int g = 0; g < D.ngroups; g++) {
      if (!bundle_group_live(D, g)) continue;
      BundleGroupCgTerm term{D, g};
      float v[2];
      S.template sum<2>(D.s.nimages, term, v);
      float diag = D.fsc[g] * bundle_fvec(D, BUNDLE_P)[g];
      if (RADIAL && bundle_radial_live(D, g)) {
        BundleGroupCgRadialTerm kterm{D, g};
        float w[2];
        S.template sum<2>(D.s.nimages, kterm, w);
        const float ufk = D.ksc[2 * BUNDLE_MAX_GROUPS + g], pk = bundle_kvec(D, BUNDLE_P)[g];
        if (lead)
          bundle_kvec(D, BUNDLE_Y)[g] = ((D.ksc[g] * pk + ufk * bundle_fvec(D, BUNDLE_P)[g]) + w[0]) - w[1];
        diag = diag + ufk * pk;
      }
      if (lead) bundle_fvec(D, BUNDLE_Y)[g] = (diag + v[0]) - v[1];
    }
    S.fence();
  }
  BundleDotTerm sterm{D.istate, D.ivec + BUNDLE_P * n6, D.ivec + BUNDLE_Y * n6};
  float sigma[1], rho2[1];
  S.template sum<1>(D.s.nimages, sterm, sigma);
  sigma[0] = bundle_dot_groups<FOCAL, RADIAL>(D, sigma[0], BUNDLE_P, BUNDLE_Y);
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
  if (FOCAL)
    for (int g = lane; g < D.ngroups; g += lanes) {
      if (!bundle_group_live(D, g)) continue;
      float *x = bundle_fvec(D, BUNDLE_X) + g, *r = bundle_fvec(D, BUNDLE_R) + g;
      x[0] = x[0] + alpha * bundle_fvec(D, BUNDLE_P)[g];
      r[0] = r[0] - alpha * bundle_fvec(D, BUNDLE_Y)[g];
      bundle_fvec(D, BUNDLE_Z)[g] = r[0] / D.fsc[BUNDLE_MAX_GROUPS + g];
    }
  if (RADIAL)
    for (int g = lane; g < D.ngroups; g += lanes) {
      if (!bundle_radial_live(D, g)) continue;
      float *x = bundle_kvec(D, BUNDLE_X) + g, *r = bundle_kvec(D, BUNDLE_R) + g;
      x[0] = x[0] + alpha * bundle_kvec(D, BUNDLE_P)[g];
      r[0] = r[0] - alpha * bundle_kvec(D, BUNDLE_Y)[g];
      bundle_kvec(D, BUNDLE_Z)[g] = r[0] / D.ksc[BUNDLE_MAX_GROUPS + g];
    }
  S.fence();
  BundleDotTerm rterm{D.istate, D.ivec + BUNDLE_R * n6, D.ivec + BUNDLE_Z * n6};
  S.template sum<1>(D.s.nimages, rterm, rho2);
  rho2[0] = bundle_dot_groups<FOCAL, RADIAL>(D, rho2[0], BUNDLE_R, BUNDLE_Z);
  const bool on = fundamental_finite(rho2[0]);
  if (on) {
    const float beta = rho2[0] / rho;
    if (FOCAL)
      for (int g = lane; g < D.ngroups; g += lanes)
        if (bundle_group_live(D, g))
          bundle_fvec(D, BUNDLE_P)[g] = bundle_fvec(D, BUNDLE_Z)[g] + beta * bundle_fvec(D, BUNDLE_P)[g];
    if (RADIAL)
      for (int g = lane; g < D.ngroups; g += lanes)
        if (bundle_radial_live(D, g))
          bundle_kvec(D, BUNDLE_P)[g] = bundle_kvec(D, BUNDLE_Z)[g] + beta * bundle_kvec(D, BUNDLE_P)[g];
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
template <bool FOCAL = false, bool RADIAL = false>
FUND_HD void bundle_track_trial(const BundleData &D, int t)
{
  if (D.ctl[BUNDLE_FAIL] || !bundle_active(D, t)) return;
  const int b = D.ctl[BUNDLE_CUR];
  float s[3], d[3];
  bundle_track_gather<FOCAL, RADIAL>(D, t, BUNDLE_X, s);
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

// FOCAL, step 5 for group g < BUNDLE_MAX_GROUPS: the trial scale s_g + x_g; one that is not finite and > 0 raises BAD
FUND_HD void bundle_focal_trial(const BundleData &D, int g)
{
  if (D.ctl[BUNDLE_FAIL]) return;
  const int b = D.ctl[BUNDLE_CUR];
  const float s = D.fs[b * BUNDLE_MAX_GROUPS + g];
  const bool live = g < D.ngroups && bundle_group_live(D, g);
  const float e = live ? s + bundle_fvec(D, BUNDLE_X)[g] : s;
  D.fs[(1 - b) * BUNDLE_MAX_GROUPS + g] = e;
  if (live && !(fundamental_finite(e) && e > 0.0f)) bundle_raise(&D.ctl[BUNDLE_BAD]);
}

// RADIAL, step 5 for group g < BUNDLE_MAX_GROUPS: the trial coefficient k_g + x_k; one that is not finite raises BAD
FUND_HD void bundle_radial_trial(const BundleData &D, int g)
{
  if (D.ctl[BUNDLE_FAIL]) return;
  const int b = D.ctl[BUNDLE_CUR];
  const float k = D.ks[b * BUNDLE_MAX_GROUPS + g];
  const bool live = g < D.ngroups && bundle_radial_live(D, g);
  const float e = live ? k + bundle_kvec(D, BUNDLE_X)[g] : k;
  D.ks[(1 - b) * BUNDLE_MAX_GROUPS + g] = e;
  if (live && !fundamental_finite(e)) bundle_raise(&D.ctl[BUNDLE_BAD]);
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
template <bool FOCAL = false, bool RADIAL = false>
FUND_HD void bundle_weight_slot(const BundleData &D, int o)
{
  const int k = D.key[o];
  float w = -1.0f;
  if (k >= 0) {
    const int b = D.ctl[BUNDLE_CUR];
    float c[12], kk[4];
    bundle_load_cam(D.cams + 12 * ((size_t)b * D.s.nimages + k), c);
    const float *P = D.pts + 3 * ((size_t)b * D.s.max_tracks + D.owner[o]);
    const float X[3] = {P[0], P[1], P[2]};
    const TrackObs ob = track_obs_load(D.s.obs + o);
    RefineView v;
    float x, y;
    bundle_observe<RADIAL>(D, D.ks + b * BUNDLE_MAX_GROUPS, k, ob, x, y);
    if (refine_view(c, bundle_intrinsics<FOCAL>(D, b, k, kk), X, x, y, v))
      w = pose_one_nan(bundle_loss(D.loss, D.loss_scale, D.loss_scale2, v.ru * v.ru + v.rv * v.rv).w);
    else
      w = pose_one_nan(NAN);                   // the final state has every member in front: not reached
  }
  D.obs_weight[o] = w;
}

// d_intrinsics_out of image i and d_focal of group g < ngroups.  `refined`: an image has a group, so the FOCAL instances
// ran; otherwise every s_g is 1, no member is counted and the intrinsics come back bit for bit
FUND_HD int bundle_focal_status(const BundleData &D, int g, bool refined)
{
  if (D.num_loops == 0) return BUNDLE_FOCAL_NOT_REFINED;
  return refined && bundle_group_live(D, g) ? BUNDLE_FOCAL_REFINED : BUNDLE_FOCAL_NO_MEMBER;
}
FUND_HD void bundle_intrinsics_out(const BundleData &D, int i, bool refined)
{
  const unsigned *given = reinterpret_cast<const unsigned *>(D.s.intrinsics) + 4 * (size_t)i;
  unsigned w[4] = {given[0], given[1], given[2], given[3]};
  const int g = D.grp ? D.grp[i] : -1;
  if (g >= 0 && refined && bundle_focal_status(D, g, true) == BUNDLE_FOCAL_REFINED && D.istate[i] != BUNDLE_NO_CAMERA) {
    const float s = D.fs[D.ctl[BUNDLE_CUR] * BUNDLE_MAX_GROUPS + g];
    const float fx = D.s.intrinsics[4 * (size_t)i] * s, fy = D.s.intrinsics[4 * (size_t)i + 1] * s;
    __builtin_memcpy(&w[0], &fx, sizeof fx);
    __builtin_memcpy(&w[1], &fy, sizeof fy);
  }
  unsigned *out = reinterpret_cast<unsigned *>(D.intrinsics_out) + 4 * (size_t)i;
  out[0] = w[0]; out[1] = w[1]; out[2] = w[2]; out[3] = w[3];
}
FUND_HD void bundle_focal_out(const BundleData &D, int g, bool refined)
{
  const float s = refined ? D.fs[D.ctl[BUNDLE_CUR] * BUNDLE_MAX_GROUPS + g] : 1.0f;
  int *out = D.focal_out + 3 * (size_t)g;
  __builtin_memcpy(&out[0], &s, sizeof s);
  out[1] = refined ? D.fcount[g] : 0;
  out[2] = bundle_focal_status(D, g, refined);
}

// d_radial of group g < ngroups.  `refined` as above; `radial`: the RADIAL instances ran, otherwise k_g is k0_g
FUND_HD void bundle_radial_out(const BundleData &D, int g, bool refined, bool radial)
{
  const float k = radial ? D.ks[D.ctl[BUNDLE_CUR] * BUNDLE_MAX_GROUPS + g] : D.k0[g];
  const int n = refined ? D.fcount[g] : 0;
  int status = BUNDLE_RADIAL_HELD;
  if (D.rad[g] && D.num_loops == 0) status = BUNDLE_RADIAL_NOT_REFINED;
  else if (D.rad[g]) status = radial && n > 0 ? BUNDLE_RADIAL_REFINED : BUNDLE_RADIAL_NO_MEMBER;
  int *out = D.radial_out + 3 * (size_t)g;
  __builtin_memcpy(&out[0], &k, sizeof k);
  out[1] = n;
  out[2] = status;
}

// misift_undistort_obs_batch, slot o < O: frame and record copied, the position under the radial model with k_g of
// d_radial when the frame is an image with a group, otherwise bit for bit
FUND_HD TrackObs bundle_undistort_obs(TrackObs ob, int nimages, const float *intrinsics, const int *group,
                                      const int *radial)
{
  if (ob.frame < 0 || ob.frame >= nimages) return ob;
  const int g = group[ob.frame];
  if (g < 0) return ob;
  float k, qu, qv;
  __builtin_memcpy(&k, &radial[3 * (size_t)g], sizeof k);
  bundle_radial_apply(intrinsics + 4 * (size_t)ob.frame, k, ob.xpos, ob.ypos, qu, qv);
  return ob;
}

// ---- the model <FOCAL, RADIAL> under one name per phase, so that no caller picks among the functions above by hand.
// Each forwards to the function of its model and holds no statement of its own: the bodies stay apart because a shared
// one moved the register allocation.  Beside them the number of sums each phase hands its Sum at once.

template <bool FOCAL, bool RADIAL>
constexpr int BUNDLE_NORMAL_SUMS = RADIAL ? BUNDLE_NORMAL_RADIAL : FOCAL ? BUNDLE_NORMAL_FOCAL : BUNDLE_NORMAL;
template <bool FOCAL, bool RADIAL>
constexpr int BUNDLE_CG_IMAGE_SUMS = RADIAL ? 8 : FOCAL ? 7 : 6;
template <bool FOCAL, bool RADIAL>
constexpr int BUNDLE_CG_START_SUMS = RADIAL ? 4 : FOCAL ? 3 : 1;
template <bool FOCAL, bool RADIAL>
constexpr int BUNDLE_CG_SCALAR_SUMS = FOCAL ? 2 : 1;

template <bool ROBUST, bool FOCAL, bool RADIAL>
FUND_HD void bundle_track_normal_of(const BundleData &D, int t)
{
  if constexpr (FOCAL) bundle_track_normal_focal<ROBUST, RADIAL>(D, t);
  else bundle_track_normal<ROBUST>(D, t);
}
template <bool FOCAL, bool RADIAL, class Sum>
FUND_HD void bundle_image_normal_of(const BundleData &D, Sum &S, int i, bool lead)
{
  if constexpr (RADIAL) bundle_image_normal_radial(D, S, i, lead);
  else if constexpr (FOCAL) bundle_image_normal_focal(D, S, i, lead);
  else bundle_image_normal(D, S, i, lead);
}
template <bool FOCAL, bool RADIAL, class Sum>
FUND_HD void bundle_cg_image_of(const BundleData &D, Sum &S, int i, bool lead)
{
  if constexpr (RADIAL) bundle_cg_image_radial(D, S, i, lead);
  else if constexpr (FOCAL) bundle_cg_image_focal(D, S, i, lead);
  else bundle_cg_image(D, S, i, lead);
}
// the trial scalars of group g < BUNDLE_MAX_GROUPS: the scale, then the coefficient
template <bool FOCAL, bool RADIAL>
FUND_HD void bundle_group_trial(const BundleData &D, int g)
{
  if constexpr (FOCAL) bundle_focal_trial(D, g);
  if constexpr (RADIAL) bundle_radial_trial(D, g);
}

// ---- the phases as stateless types, by the shape of their work item: what the kernels (kernels_bundle.hip) and the
// loops of the hook (bundle_host.hpp) are instantiated over, and what the schedule (bundle_host.hpp) names.  `run` is
// the function of the phase itself where it takes (D, work item, flag of the launch ...), so a kernel calls it as
// directly as a kernel written by hand would (a forwarding function in between moved one instruction of the robust
// cost pass); where the function is a template over the Sum, run forwards to it and holds no other statement.

// lane per slot o < O
template <bool RADIAL>
struct BundlePremember {
  static constexpr auto run = &bundle_slot_premember<RADIAL>;
};
template <bool ROBUST, bool FOCAL, bool RADIAL>
struct BundleEval {
  static constexpr auto run = &bundle_eval_slot<ROBUST, FOCAL, RADIAL>;   // (D, o, trial)
};
template <bool FOCAL, bool RADIAL>
struct BundleWeightOut {
  static constexpr auto run = &bundle_weight_slot<FOCAL, RADIAL>;
};

// lane per track t < T
struct BundleActivate {
  static constexpr auto run = &bundle_track_activate;
};
template <bool ROBUST, bool FOCAL, bool RADIAL>
struct BundleTrackNormal {
  static constexpr auto run = &bundle_track_normal_of<ROBUST, FOCAL, RADIAL>;
};
template <bool FOCAL, bool RADIAL>
struct BundleCgTrack {
  static constexpr auto run = &bundle_cg_track<FOCAL, RADIAL>;
};
template <bool FOCAL, bool RADIAL>
struct BundleTrackTrial {
  static constexpr auto run = &bundle_track_trial<FOCAL, RADIAL>;
};
struct BundleTrackOut {
  static constexpr auto run = &bundle_track_out;
};

// lane per image i < nimages; with GROUPS the first groups(D) lanes of the launch take a group each as well
struct BundleImageInit {
  static constexpr bool GROUPS = false;
  static constexpr auto run = &bundle_image_init;
};
template <bool FOCAL, bool RADIAL>
struct BundleImageTrial {
  static constexpr bool GROUPS = FOCAL;
  static FUND_HD int groups(const BundleData &) { return BUNDLE_MAX_GROUPS; }
  static constexpr auto run = &bundle_image_trial;
  static constexpr auto group = &bundle_group_trial<FOCAL, RADIAL>;
};
struct BundleImageOut {
  static constexpr bool GROUPS = false;
  static constexpr auto run = &bundle_image_out;
};
struct BundleIntrinsicsOut {                   // d_intrinsics_out, and d_focal of the ngroups groups
  static constexpr bool GROUPS = true;
  static FUND_HD int groups(const BundleData &D) { return D.ngroups; }
  static constexpr auto run = &bundle_intrinsics_out;   // (D, i, refined)
  static constexpr auto group = &bundle_focal_out;      // (D, g, refined)
};

// workgroup (or loop) per image with SUMS sums at once: run<Sum>(D, S, i, lead, flag of the launch ...)
struct BundleCost {
  static constexpr int SUMS = 1;
  template <class Sum>
  static FUND_HD void run(const BundleData &D, Sum &S, int i, bool lead, int trial)
  {
    bundle_image_cost(D, S, i, trial != 0, lead);
  }
};
template <bool FOCAL, bool RADIAL>
struct BundleImageNormal {
  static constexpr int SUMS = BUNDLE_NORMAL_SUMS<FOCAL, RADIAL>;
  template <class Sum>
  static constexpr auto run = &bundle_image_normal_of<FOCAL, RADIAL, Sum>;
};
template <bool FOCAL, bool RADIAL>
struct BundleCgImage {
  static constexpr int SUMS = BUNDLE_CG_IMAGE_SUMS<FOCAL, RADIAL>;
  template <class Sum>
  static constexpr auto run = &bundle_cg_image_of<FOCAL, RADIAL, Sum>;
};

// the scalar workgroup (or one pass of the hook) with SUMS sums at once: run<Sum>(D, S, lane, lanes, lead)
struct BundleStart {
  static constexpr int SUMS = 1;
  template <class Sum>
  static FUND_HD void run(const BundleData &D, Sum &S, int, int, bool lead)
  {
    bundle_scalar_init(D, S, lead);
  }
};
template <bool RADIAL>
struct BundleGroupInit {                       // takes no sum: the Sum it is handed has no memory
  static constexpr int SUMS = 0;
  template <class Sum>
  static FUND_HD void run(const BundleData &D, Sum &S, int lane, int lanes, bool)
  {
    bundle_focal_init<RADIAL>(D, S, lane, lanes);
  }
};
template <bool FOCAL, bool RADIAL>
struct BundleCgStart {
  static constexpr int SUMS = BUNDLE_CG_START_SUMS<FOCAL, RADIAL>;
  template <class Sum>
  static constexpr auto run = &bundle_cg_start<FOCAL, RADIAL, Sum>;
};
template <bool FOCAL, bool RADIAL>
struct BundleCgScalar {
  static constexpr int SUMS = BUNDLE_CG_SCALAR_SUMS<FOCAL, RADIAL>;
  template <class Sum>
  static constexpr auto run = &bundle_cg_scalar<FOCAL, RADIAL, Sum>;
};
struct BundleDecide {
  static constexpr int SUMS = 1;
  template <class Sum>
  static constexpr auto run = &bundle_decide<Sum>;
};

// ---- the host's side: the Sum as a loop

struct BundleHostSum {
  float p[BUNDLE_NORMAL_RADIAL * FUND_SLOTS];
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
