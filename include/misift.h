/* misift.h — the thin C-ABI between host code (C++ shim, ctypes, cgo, JNI …)
 * and the gfx950 HIP kernels of libmisift.so.
 *
 * Plain pointers and sizes only: no C++ types, no torch types, no HIP types
 * (a hipStream_t crosses as void*).  Every function returns 0 on success or a
 * negative MISIFT_E* code; misift_last_error() gives the message for the
 * calling thread.  Device pointers are ordinary HBM pointers (hipMalloc,
 * torch tensors' data_ptr(), …).
 *
 * Each entry point names the reference interface it replaces (file:line in
 * Celebrandil/CudaSift).  The C++ drop-in layer (include/cudaSift.h,
 * include/cudaImage.h, cudasift_amd/csrc/shim_cudasift.cpp) is written
 * purely on top of this file.
 */
#ifndef MISIFT_H
#define MISIFT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MISIFT_OK          0
#define MISIFT_EINVAL     -1   /* bad argument                                  */
#define MISIFT_EHIP       -2   /* HIP runtime / kernel launch failure           */
#define MISIFT_ENOMEM     -3   /* allocation failure                            */
#define MISIFT_ENODEV     -4   /* no gfx950 device visible                      */

#define MISIFT_NUM_SCALES      5   /* DoG scales searched per octave (cudaSiftD.h:8) */
#define MISIFT_MAX_OCTAVES     7   /* counter protocol has 17 slots = 2*8+1          */
#define MISIFT_POINT_BYTES   576   /* sizeof(SiftPoint) (cudaSift.h:6-22)            */

/* Same 576-byte record as SiftPoint in include/cudaSift.h (reference
 * cudaSift.h:6-22); declared here so C callers need no C++ header. */
typedef struct misift_point {
  float xpos, ypos, scale, sharpness, edgeness, orientation, score, ambiguity;
  int32_t match;
  float match_xpos, match_ypos, match_error, subsampling;
  float empty[3];
  float data[128];
} misift_point;

typedef struct misift_ctx misift_ctx;   /* opaque: one per device (+stream)  */

/* Behaviour switches.  Defaults reproduce the reference. */
typedef struct misift_options {
  int texfrac_bits;      /* 8 = emulate CUDA's 9-bit texture filter weights
                            (cudaSiftH.cu:196-205); 23 = full fp32 bilinear   */
  int fix_numpts;        /* 0 = numPts excludes finest-octave duplicates
                            (cudaSiftH.cu:115); 1 = include them              */
  int match_full;        /* 0 = ignore the last n2%32 columns
                            (matching.cu:325); 1 = use every column           */
  int match_exact_top2;  /* 0 = 8-class lossy runner-up merge
                            (matching.cu:378-390); 1 = true second best       */
  int quiet;             /* 1 = C++ shim prints nothing per call              */
  int fused;             /* 1 = fused DoG+extrema kernel (no DoG planes in
                            HBM); 0 = separate laplace / findpoints kernels   */
  int deterministic;     /* 0 = records in atomic-append order within an octave
                            segment, like the reference (cudaSiftD.cu:1420,
                            :1043: run-to-run the SET is equal, the order is
                            not); 1 = order fixed by the keypoints themselves
                            (tile, y, x, scale): repeated runs are byte-identical
                            (also MISIFT_DETERMINISTIC=1).
                            The fused path orders by (tile, y, x, scale); the
                            dense kernels (fused = 0, or the automatic exact
                            re-run after a candidate-list overflow) sort every
                            segment by (y, x, scale, orientation) afterwards   */
  int reference_cap;     /* 0 = every scale-space extremum goes on to the refinement
                            (ours); 1 = the reference's cap: a block of
                            FindPointsMultiNew — 30 columns x 8 rows of one scale —
                            keeps its first 32 extrema (by column, then row) and
                            drops the rest (cudaSiftD.cu:1369-1377; SURVEY
                            Appendix B #4).  Natural images never reach 32 per
                            240 pixels.  Costs nothing since r06: the fused path
                            counts the true extrema of every block and only a
                            frame in which one reaches a 33rd is redone on the
                            dense per-level kernels, which apply the cap in the
                            reference's order.  The cudaSift.h shim switches it ON
                            (reference-identical by default); the C-ABI default is
                            0 (also MISIFT_REFERENCE_CAP=1)                      */
} misift_options;

/* ------------------------------------------------------------------ runtime */

/* cudaSiftH.cu:19-37 (InitCuda): device count / properties. */
int misift_device_count(void);
int misift_device_info(int device, char *name, int name_len, int *mem_clock_khz,
                       int *bus_width_bits, size_t *total_mem_bytes,
                       int *num_cus, int *lds_bytes_per_block);
/* ISA name of the device ("gfx950:sramecc+:xnack-"); the shim uses it to print the right HBM data rate. */
int misift_device_arch(int device, char *arch, int arch_len);

/* hipGraph replay of repeated synchronous calls: when misift_extract / misift_extract_batch is called again
 * with exactly the same arguments and buffers (the reference demo does, mainSift.cpp:64-69), the launch
 * sequence is captured on the 2nd occurrence and replayed afterwards as one hipGraphLaunch.  OFF by default:
 * on ROCm 7.2 / MI355X the replay measured SLOWER than the ~10 direct launches (single 1080p frame 0.199 ms vs
 * 0.170 ms; 64-frame batch 1.508 vs 1.502 ms).  Also MISIFT_GRAPH=1 in the environment at context creation. */
int misift_ctx_set_graph_replay(misift_ctx *ctx, int on);

/* One context per device; `stream` is a hipStream_t (NULL = the null stream).
 * The context owns the per-frame point counters (cudaSiftD.cu:13-14), a
 * pinned read-back buffer and the filter tap tables (cudaSiftD.cu:15-17). */
int misift_ctx_create(int device, void *stream, misift_ctx **out);
void misift_ctx_destroy(misift_ctx *ctx);
/* Moves the context to another hipStream_t (NULL = the null stream).  The context stays ONE in-order pipeline across the
 * switch: its temp memory, its pair plan, its pinned ring of host lists and its counters belong to the context, not to a
 * stream, so work enqueued through the context after the call starts behind everything enqueued through it before (an
 * event of the context's is recorded on the old stream and the new stream waits for it).  The call does not wait on the
 * host, and the caller's old stream may be destroyed once its work is done.  Switching to the stream the context is
 * already on does nothing.  ctx NULL: MISIFT_EINVAL.  The event is recorded when the call is made, so whatever the
 * caller itself had put on the old stream by then is waited for as well, and what it puts there afterwards is not.
 * Out of scope: a switch while misift_ctx_set_batches_in_flight(K > 1) pipelines or a misift_pipe on this context are
 * active (drain them first), and graph replay (a captured graph belongs to the stream it was captured for). */
int misift_ctx_set_stream(misift_ctx *ctx, void *stream);
/* Synchronous calls return at the last kernel's completion flag (1) instead of after a stream synchronisation (0, the
 * default): see misift_extract.  The host polls a word of pinned memory, i.e. it spins a core while it waits. */
int misift_ctx_set_early_return(misift_ctx *ctx, int on);
/* Diagnostics: calls this context re-ran with a stand-alone ScaleDown chain launch because the bounded in-launch wait
 * of the single-call path expired (never on a healthy device; MISIFT_CHAIN_WAIT_US sets the bound, default 100000). */
int misift_ctx_chain_fallbacks(misift_ctx *ctx);
/* Diagnostics: calls this context re-ran with separate orientation and descriptor launches because the bounded in-launch
 * wait of the fused kernel of the single-call path (r06) expired (never on a healthy device; MISIFT_FUSE_WAIT_US sets the
 * bound, default 100000; MISIFT_FUSE_ORIENT=0 keeps the two launches). */
int misift_ctx_fuse_fallbacks(misift_ctx *ctx);
/* Diagnostics: 1 if the last extraction enqueued on this context dealt the workgroups of its per-keypoint kernels out
 * in proportion to the frames' keypoint counts (batches of more than MISIFT_SMALL_FRAMES frames, MISIFT_BALANCE != 0). */
int misift_ctx_last_call_balanced(misift_ctx *ctx);
/* Diagnostics: synchronous calls of a frame or two whose descriptor launch was the last one (r05) but that then needed the
 * global-memory descriptor kernel after all, for a keypoint larger than the LDS window (next to never; MISIFT_FOLD_TAIL=0
 * always launches it). */
int misift_ctx_descr_big_fallbacks(misift_ctx *ctx);
int misift_ctx_sync(misift_ctx *ctx);
const char *misift_last_error(void);

void misift_default_options(misift_options *opt);
/* misift_options grows at its END (reference_cap was added in r05) and has no size member, so the caller's sizeof
 * travels with the call: the _sized entry points copy min(struct_size, the library's sizeof) bytes — fields the caller's
 * header does not know keep their current value (set) / are not written (get) — and nothing is read or written past the
 * caller's struct.  Code compiled against THIS header gets them through the two macros below; the plain exported
 * symbols stay for binaries built against the r04 header and touch the seven fields that header had, no more. */
void misift_default_options_sized(misift_options *opt, size_t struct_size);
int misift_set_options_sized(misift_ctx *ctx, const misift_options *opt, size_t struct_size);
int misift_get_options_sized(misift_ctx *ctx, misift_options *opt, size_t struct_size);
int misift_set_options(misift_ctx *ctx, const misift_options *opt);
int misift_get_options(misift_ctx *ctx, misift_options *opt);
#ifndef MISIFT_NO_OPTION_MACROS
#define misift_default_options(opt) misift_default_options_sized((opt), sizeof(*(opt)))
#define misift_set_options(ctx, opt) misift_set_options_sized((ctx), (opt), sizeof(*(opt)))
#define misift_get_options(ctx, opt) misift_get_options_sized((ctx), (opt), sizeof(*(opt)))
#endif

/* ------------------------------------------------------------------- memory */

/* cudaMalloc / cudaFree / cudaMemcpy as used by cudaSiftH.cu:234-264 and
 * cudaImage.cu:15-78. */
int misift_malloc(size_t bytes, void **out);
int misift_free(void *ptr);
int misift_memset(misift_ctx *ctx, void *ptr, int value, size_t bytes);
int misift_copy_h2d(misift_ctx *ctx, void *dst, const void *src, size_t bytes);
int misift_copy_d2h(misift_ctx *ctx, void *dst, const void *src, size_t bytes);
/* cudaMallocPitch: rows padded to a multiple of 128 floats (cudaImage.cu:24). */
int misift_image_alloc(int width, int height, float **d_out, int *pitch_floats);
/* cudaMemcpy2D, all strides in floats (cudaImage.cu:55-78). */
int misift_upload_2d(misift_ctx *ctx, float *d_dst, int dpitch, const float *h_src,
                     int hpitch, int width, int height);
int misift_download_2d(misift_ctx *ctx, float *h_dst, int hpitch, const float *d_src,
                       int dpitch, int width, int height);
/* Strided gather of `nfields` consecutive 32-bit fields starting at byte
 * `offset` of every 576-byte record (matching.cu:1195-1199). */
int misift_download_fields(misift_ctx *ctx, void *h_pts, const void *d_pts, int npts,
                           int offset, int nfields);

/* Scratch arena: cudaSiftH.cu:39-64 (AllocSiftTempMemory). Size in floats. */
size_t misift_scratch_floats(int width, int height, int num_octaves, int scale_up);

/* --------------------------------------------------------------- extraction */

/* cudaSiftH.cu:72-144 (ExtractSift) for one device-resident frame.
 * d_img: width x height floats, row stride `pitch` floats.  Any float-aligned base and any pitch >= width are accepted —
 *   a sub-rectangle &img[y0 * pitch + x0] of a larger image with the parent's pitch, an odd pitch — and nothing outside
 *   the width x height pixels influences the result (the source is only read, and never past the end of a row's pitch).
 *   A base aligned to 16 bytes with a pitch that is a multiple of 4 floats selects the vector-load kernels; anything else
 *   runs the generic ones: same records, bit for bit.
 * d_scratch: misift_scratch_floats() floats, or NULL to allocate per call.  Any float-aligned pointer is accepted (an
 *   arena carved out of a pool at any offset); a 16-byte aligned one (any hipMalloc pointer, or one at a multiple of 4
 *   floats inside a pool) selects the vector kernels inside the arena, anything else the generic ones: same pyramid and
 *   same records, bit for bit.  Nothing is written in front of d_scratch or behind its misift_scratch_floats() floats.
 * d_pts: max_pts records.  *num_pts_out follows the reference's rule
 * numPts = min(counter[2*num_octaves], max_pts) (cudaSiftH.cu:115-116).
 * max_pts is a capacity, not a selection.  Let c be the 17 counters an unlimited call would leave (misift_get_counters:
 *   the detections of octave k, coarsest k = 1, are the rows [c[2k-1], c[2k]), its second orientations the rows
 *   [c[2k], c[2k+1])).  With any max_pts >= 1, and for every frame of every batch call below alike:
 *   - numPts = min(c[2*num_octaves], max_pts), with options.fix_numpts min(c[2*num_octaves+1], max_pts); the packed
 *     call's d_counts_out[f] is the same number.
 *   - The rows [0, min(c[2*num_octaves+1], max_pts)) of d_pts hold records — this includes the finest octave's second
 *     orientations behind numPts when fix_numpts is 0 — and no row behind them, no row of another frame and no packed
 *     record behind d_offsets_out[nframes] is written.  A segment that ends at or below max_pts holds exactly the records
 *     it holds in the unlimited call.  The one segment that contains row max_pts holds max_pts - start distinct records of
 *     that same segment of the unlimited call, each complete and equal to what it is there (scale_up: halved exactly once
 *     inside numPts); WHICH of the segment's records they are follows the append order and may differ from run to run
 *     and from the reference's choice.  Everything behind row max_pts is dropped, never moved forward.
 *   - A dropped record is still counted: every counter word whose unlimited value is below max_pts has that value, every
 *     other word is >= max_pts, and the per-octave detection counts c[2k] - c[2k-1] are those of the unlimited call.  The
 *     duplicate counts from the cut on are not specified: a dropped detection may get no orientation.
 *   - options.deterministic = 1 at capacity: repeated calls are byte-identical over [0, numPts) on every frame whose
 *     per-octave detection counts are all <= max_pts (the fused path stages each octave's detections in a list of
 *     max_pts entries and orders the list before anything is cut).  Where an octave's list itself overflows, which
 *     detections it keeps is the append order again and only the rule above holds.  The dense kernels (fused = 0, or the
 *     exact re-run after a candidate-list overflow) have no staging list — they append to d_pts itself and order its
 *     segments afterwards — so there the promise covers the frames in which no segment inside numPts is cut, i.e. whose
 *     unlimited numPts is <= max_pts.
 * One host<->device sync (the count read-back), like the reference.
 * Completion: the call returns after the context's stream has been synchronised — every record is written and visible
 * to any stream, device or host copy, like the reference's blocking ExtractSift.  misift_ctx_set_early_return(ctx, 1)
 * (r05: opt-in; it was the default in r04) lets the synchronous calls return as soon as the call's last kernel has
 * handed the counts to the host through pinned memory (~10 us earlier): the records are then ordered only for work
 * enqueued on the CONTEXT'S stream afterwards (misift_match, misift_copy_d2h, the cudaSift.h shim's read-back);
 * a consumer on another stream or device must call misift_ctx_sync() first.  MISIFT_HOST_SPIN=0 / =1 in the
 * environment overrides either way.  The same holds for misift_match / misift_match_rows.
 * Any size from 1 x 1 and any num_octaves <= MISIFT_MAX_OCTAVES is accepted, like the reference (cudaSiftH.cu:72-167):
 * images under 16 x 16, or whose coarsest pyramid level is under 8 px, run on the dense per-level kernels (every access
 * clamped); a level that integer division has shrunk to 0 pixels is empty and skipped (tests/test_gpu_refemul.py:
 * same numPts, counters and keypoints as the emulated reference down to 1 x 1).  Only width, height < 16384
 * (after the doubling of scale_up) and max_pts >= 1 are required, else MISIFT_EINVAL. */
int misift_extract(misift_ctx *ctx, const float *d_img, int width, int height, int pitch,
                   int num_octaves, float init_blur, float thresh, float lowest_scale,
                   int scale_up, float *d_scratch, void *d_pts, int max_pts,
                   int *num_pts_out);

/* Same pipeline over a batch of independent frames in one launch sequence
 * (BASELINE config 4: frames shard across GPUs, one batch per device).
 * d_imgs: nframes images, frame stride `frame_stride` floats.  Base and pitch as for misift_extract; any frame_stride is
 *   accepted (frames with a gap between them, frames of a larger parent, a stride that is no multiple of 4).  The
 *   vector-load kernels need a 16-byte aligned base and pitch and frame_stride multiples of 4 floats — for 8-bit frames
 *   (misift_extract_batch_u8 / _ex) a 4-byte aligned base and pitch and frame_stride multiples of 4 bytes; anything else
 *   runs the generic kernels with the same records, bit for bit.  The same holds for every batch call below.
 * d_scratch: nframes * misift_scratch_floats() floats (or NULL); any float-aligned pointer, as for misift_extract.
 * d_pts: nframes * max_pts records, frame f at d_pts + f*max_pts.
 * num_pts_out: host array of nframes ints. */
int misift_extract_batch(misift_ctx *ctx, const float *d_imgs, int nframes,
                         size_t frame_stride, int width, int height, int pitch,
                         int num_octaves, float init_blur, float thresh,
                         float lowest_scale, float *d_scratch, void *d_pts,
                         int max_pts, int *num_pts_out);
/* As above but does not synchronise: counts stay on the device
 * (d_counts_out: nframes ints, may be NULL) so a caller can queue batches. */
int misift_extract_batch_async(misift_ctx *ctx, const float *d_imgs, int nframes,
                               size_t frame_stride, int width, int height, int pitch,
                               int num_octaves, float init_blur, float thresh,
                               float lowest_scale, float *d_scratch, void *d_pts,
                               int max_pts, int *d_counts_out);

/* As misift_extract_batch_async, and additionally packs the valid records of all
 * frames contiguously (frame after frame) into d_packed_out, ready for ONE
 * device-to-device / xGMI / PCIe transfer: d_counts_out[f] = numPts of frame f
 * (-1: that frame's candidate list overflowed), d_offsets_out[0..nframes] =
 * exclusive prefix sum of the non-negative counts (records).  In the default
 * (fused) mode the descriptor kernel writes the packed array itself — no extra
 * packing pass — and d_pts may be NULL (if given it is filled as well); calls
 * that run on the dense kernels (fused = 0, reference_cap, images under 16 x 16
 * or with a coarsest level under 8 px) need d_pts (MISIFT_EINVAL otherwise).  Nothing
 * synchronises; this is what the multi-GPU gather of SiftData (BASELINE
 * config 4) and the host pipeline send. */
int misift_extract_batch_packed_async(misift_ctx *ctx, const float *d_imgs, int nframes,
                                      size_t frame_stride, int width, int height, int pitch,
                                      int num_octaves, float init_blur, float thresh,
                                      float lowest_scale, float *d_scratch, void *d_pts,
                                      int max_pts, int *d_counts_out, int *d_offsets_out,
                                      void *d_packed_out);

/* As misift_extract_batch, but the frames are 8-bit (pitch and frame_stride in
 * bytes): the prefilter converts in registers, so the result is bit-identical
 * to an fp32 upload of the same pixel values (what mainSift.cpp:41-42 does on
 * the host with convertTo(CV_32FC1)) at a quarter of the PCIe and HBM read bytes. */
int misift_extract_batch_u8(misift_ctx *ctx, const unsigned char *d_imgs, int nframes,
                            size_t frame_stride, int width, int height, int pitch,
                            int num_octaves, float init_blur, float thresh,
                            float lowest_scale, float *d_scratch, void *d_pts,
                            int max_pts, int *num_pts_out);

/* ExtractSift's whole argument surface over a batch: 8-bit or fp32 frames (src_u8; pitch and frame_stride in source
 * elements) and scaleUp (cudaSiftH.cu:118-132: every frame is doubled first, lowestScale doubles, positions and
 * scales are halved at the end).  d_scratch: nframes * misift_scratch_floats(width, height, num_octaves, scale_up). */
int misift_extract_batch_ex(misift_ctx *ctx, const void *d_imgs, int src_u8, int nframes, size_t frame_stride,
                            int width, int height, int pitch, int num_octaves, float init_blur, float thresh,
                            float lowest_scale, int scale_up, float *d_scratch, void *d_pts, int max_pts,
                            int *num_pts_out);

/* ------------------------------------------------- host-fed pipeline
 * Streams batches of HOST frames through upload -> extraction -> read-back on three
 * HIP streams, replacing the blocking CudaImage::Download (cudaImage.cu:55-66) and the
 * blocking SiftPoint read-back of ExtractSift (cudaSiftH.cu:139-140).  Frames are tightly
 * packed (row stride = width, as CudaImage::Download assumes for h_data), fp32 or 8-bit.
 * Up to `depth` batches may be in flight; batches are collected in submission order.
 *   misift_pipe_submit   enqueues upload + extraction of `nframes` (<= batch_frames) frames and
 *                        returns at once; host_frames must stay valid until the batch is
 *                        collected (pinned memory from misift_host_alloc makes the upload async).
 *   misift_pipe_collect  waits for the oldest batch: counts_out[f] = numPts of frame f; the valid
 *                        records of all frames, frame after frame, are copied to host_records
 *                        (capacity in records; may be NULL to skip).  If a candidate list of the
 *                        fused scan overflowed, the batch is redone here with the exact dense
 *                        kernels (as misift_extract_batch does): nothing is dropped silently. */
typedef struct misift_pipe misift_pipe;
int misift_pipe_create(misift_ctx *ctx, int width, int height, int batch_frames, int src_u8,
                       int num_octaves, float init_blur, float thresh, float lowest_scale,
                       int max_pts, int depth, misift_pipe **out);
void misift_pipe_destroy(misift_pipe *pipe);
int misift_pipe_submit(misift_pipe *pipe, const void *host_frames, int nframes);
int misift_pipe_collect(misift_pipe *pipe, int *nframes_out, int *counts_out, void *host_records,
                        size_t capacity_records, size_t *nrecords_out);
int misift_pipe_pending(const misift_pipe *pipe);
/* Pinned host memory for frames / records (truly asynchronous copies). */
int misift_host_alloc(size_t bytes, void **out);
int misift_host_free(void *ptr);

/* Per-frame point counters of the last extraction, 17 per frame, in the
 * reference's layout (cudaSiftD.cu:14, protocol cudaSiftD.cu:1297-1300). */
int misift_get_counters(misift_ctx *ctx, int frame, unsigned int *counters17);
/* Diagnostic: all 64 words of one frame's counter block (the 17 reference counters, then per-octave candidate /
 * detection / duplicate counts and overflow flags); frame == frames of the last call: the call's flag block. */
int misift_get_counter_block(misift_ctx *ctx, int frame, unsigned int *words64);
int misift_set_counters(misift_ctx *ctx, int frame, const unsigned int *counters17);

/* ------------------------------------------------- stage-level entry points
 * The individual launch wrappers of cudaSiftH.cu:308-514, exposed so each
 * kernel can be checked against the oracle in isolation. */

/* LowPass (cudaSiftH.cu:406-435, LowPassBlock cudaSiftD.cu:1986-2037). */
int misift_lowpass(misift_ctx *ctx, const float *d_src, int width, int height, int spitch,
                   float *d_dst, int dpitch, float sigma);
/* LowPass and the first ScaleDown of the pyramid in one pass (what ExtractSift does
 * back to back, cudaSiftH.cu:112 + :153-154): dst = LowPass(src), dst2 = ScaleDown(dst),
 * bit-identical to the two separate calls.  Needs 16-byte aligned rows of d_src and d_dst (base, and pitch % 4 == 0) and
 * 8-byte aligned rows of d_dst2 (base, and dpitch2 % 2 == 0): MISIFT_EINVAL otherwise, nothing is written
 * (misift_extract falls back to the separate kernels by itself).  Any width >= 4 (since r03) and height >= 8; only the
 * width x height and (width/2) x (height/2) pixels of the destinations are written. */
int misift_lowpass_scaledown(misift_ctx *ctx, const float *d_src, int width, int height, int spitch,
                             float *d_dst, int dpitch, float sigma, float *d_dst2, int dpitch2);
/* ScaleDown (cudaSiftH.cu:308-338, cudaSiftD.cu:84-168): dst is (w/2,h/2). */
int misift_scaledown(misift_ctx *ctx, const float *d_src, int width, int height,
                     int spitch, float *d_dst, int dpitch);
/* ScaleUp (cudaSiftH.cu:340-351, cudaSiftD.cu:170-190): dst is (2w,2h).  dpitch must be even (MISIFT_EINVAL otherwise);
 * d_dst itself may sit at any float offset. */
int misift_scaleup(misift_ctx *ctx, const float *d_src, int width, int height, int spitch,
                   float *d_dst, int dpitch);
/* PrepareLaplaceKernels (cudaSiftH.cu:439-458): fills 8*12*16 floats. */
int misift_laplace_taps(int num_octaves, float *taps_8x12x16);
/* LaplaceMulti (cudaSiftH.cu:460-487, LaplaceMultiMem cudaSiftD.cu:1753-1793):
 * 7 DoG planes, plane stride height*pitch.  `octave` = reference octave index
 * (num_octaves = finest … 1 = coarsest) selecting the tap table. */
int misift_laplace(misift_ctx *ctx, const float *d_base, int width, int height, int pitch,
                   int num_octaves, int octave, float *d_dog);
/* FindPointsMulti (cudaSiftH.cu:489-514, FindPointsMultiNew cudaSiftD.cu:1292-1431).
 * Appends to d_pts using the context counters of frame 0 (reset them with
 * misift_reset_counters first). */
int misift_reset_counters(misift_ctx *ctx, int max_pts);
int misift_findpoints(misift_ctx *ctx, const float *d_dog, int width, int height, int pitch,
                      float thresh, float edge_limit, float lowest_scale,
                      float subsampling, int octave, void *d_pts, int max_pts);
/* Fused LaplaceMulti + FindPointsMulti: same result, no DoG planes in HBM. */
int misift_dog_findpoints(misift_ctx *ctx, const float *d_base, int width, int height,
                          int pitch, int num_octaves, int octave, float thresh,
                          float edge_limit, float lowest_scale, float subsampling,
                          void *d_pts, int max_pts);
/* ComputeOrientations (cudaSiftH.cu:353-369, cudaSiftD.cu:972-1057). */
int misift_orientations(misift_ctx *ctx, const float *d_base, int width, int height,
                        int pitch, int octave, void *d_pts, int max_pts);
/* ExtractSiftDescriptors (cudaSiftH.cu:371-382, cudaSiftD.cu:308-417). */
int misift_descriptors(misift_ctx *ctx, const float *d_base, int width, int height,
                       int pitch, float subsampling, int octave, void *d_pts, int max_pts);
/* RescalePositions (cudaSiftH.cu:397-404, cudaSiftD.cu:753-761). */
int misift_rescale_positions(misift_ctx *ctx, void *d_pts, int npts, float scale);

/* ----------------------------------------------------------------- matching */

/* MatchSiftData (matching.cu:1090-1206; CleanMatches :289, FindMaxCorr10
 * :301-397) on device-resident records: fills score, ambiguity, match,
 * match_xpos, match_ypos of d_pts1[0..n1).  fp32 MFMA, k-ordered so every
 * score is bit-identical to the reference's sequential FMA chain. */
int misift_match(misift_ctx *ctx, void *d_pts1, int n1, const void *d_pts2, int n2);
/* Row-block form for BASELINE config 5: rows [row_begin,row_begin+row_count)
 * of set 1 against all of set 2 (each GPU takes one row block). */
int misift_match_rows(misift_ctx *ctx, void *d_pts1, int row_begin, int row_count,
                      const void *d_pts2, int n2);
/* Batched pair matching (no reference counterpart; the C++ drop-in headers, cudaSift.h, do not change): for each pair
 * i, MatchSiftData(frame pairs[2i] of set 1, frame pairs[2i+1] of set 2), stream-ordered on the context stream, with
 * no host synchronisation and no host read of the counts.
 * Frame f of a set: its records start at d_recs + d_offsets[f] (d_offsets NULL: at f * stride records), and it holds
 * max(d_counts[f], 0) of them (-1 = an overflowed frame = no records) — the layout misift_extract_batch_packed_async
 * leaves, or a padded one (d_offsets NULL, stride = max_pts).  Fills score, ambiguity, match, match_xpos, match_ypos of
 * set 1's records exactly as misift_match on that pair would, in every misift_options match mode; match indices are
 * frame-local.  A pair with n1 == 0 or n2 == 0 leaves its set-1 records untouched (matching.cu:1095-1096).
 *   - The call returns before the GPU work is done.  `pairs` (npairs x 2 ints) is host memory the library copies: the
 *     caller may reuse it at once.
 *   - d_recs1 == d_recs2 is allowed (frame f against frame f + 1 of one packed batch): the call reads only descriptors
 *     and xpos / ypos, and writes only the five match fields.
 *   - A set-1 frame may appear in at most one pair.  npairs < 0, a frame index outside [0, nframes) of its set or a
 *     repeated set-1 frame: MISIFT_EINVAL, before anything is enqueued.  npairs == 0: nothing happens.
 *   - Three launches whatever npairs (plan, sweep, merge of chunked columns); nothing is sized by max_pts.
 *   - Directly behind misift_extract_batch_packed_async on the same context (K = 1) no synchronisation is needed.  With
 *     K > 1 batches in flight the extraction does not run on the context stream: order the call behind it with
 *     misift_ctx_wait_batch / misift_ctx_record_batch (see below). */
int misift_match_batch(misift_ctx *ctx, int npairs, const int *pairs,
                       void *d_recs1, int nframes1, const int *d_counts1, const int *d_offsets1, int stride1,
                       const void *d_recs2, int nframes2, const int *d_counts2, const int *d_offsets2, int stride2);
/* Pair-indexed batch matching (no reference counterpart): the pairs, frames, layouts (d_offsets or stride), count -1 and
 * stream semantics of misift_match_batch, but pair i writes its own output rows instead of the set-1 records, so that
 * frames may repeat: windowed (f against f + 1 ... f + W), keyframe and exhaustive matching in one call.  For pair
 * i = (f1, f2), n1 = max(count1[f1], 0) and n2 = max(count2[f2], 0).
 *   - A set-1 frame and a set-2 frame may appear in any number of pairs; (f, f) and d_recs1 == d_recs2 are allowed.
 *     Nothing in d_recs1 or d_recs2 is written.
 *   - n1 > max_pts or n2 > max_pts: d_out_counts[i] = -1 and d_num_matched[i] = -1; none of the pair's output bytes is
 *     written.  Otherwise d_out_counts[i] = n1, and output row r < n1 of pair i is the record d_out + (i * max_pts + r),
 *     of which exactly seven fields are written: xpos and ypos (set-1 record r's), and score, ambiguity, match,
 *     match_xpos, match_ypos, bit-identical to what misift_match on that pair writes into set-1 record r under the
 *     context's match_full / match_exact_top2 options (what misift_match_batch writes).  n2 == 0: every row is a
 *     no-match row (score 0, ambiguity 0, match -1, match_xpos 0, match_ypos 0).  Every other byte of d_out is untouched.
 *   - mutual = 1 (cross-check): a row r with forward match m >= 0 keeps it only if r is the best row of column m over
 *     all n1 rows — the largest score S_rm > 0, the smallest row on a tie: the match misift_match with the sets swapped
 *     writes for set-2 record m in match_full + match_exact_top2 mode; otherwise it becomes a no-match row.  mutual = 0:
 *     no filter.
 *   - d_num_matched (may be NULL): per pair, the output rows with match >= 0 after the filter.
 *   - The output is a batch the homography calls take as it is: frame i = pair i, d_offsets NULL, stride = max_pts,
 *     counts = d_out_counts (misift_find_homography_batch, misift_improve_homography_batch).
 *   - npairs < 0, a frame index outside [0, nframes) of its set, a NULL records, counts or output pointer, max_pts < 1,
 *     mutual other than 0 or 1, d_out equal to d_recs1 or d_recs2: MISIFT_EINVAL, before anything is enqueued.
 *     npairs == 0: nothing happens.
 *   - The call returns before the GPU work is done.  `pairs` is host memory the library copies.  Three launches and,
 *     with mutual, one memset, whatever npairs (plan, sweep, finalize); temp memory is sized from npairs, max_pts and
 *     the CU count only.  Ordering behind batches in flight (K > 1): as misift_match_batch. */
int misift_match_pairs_batch(misift_ctx *ctx, int npairs, const int *pairs,
                             const void *d_recs1, int nframes1, const int *d_counts1, const int *d_offsets1, int stride1,
                             const void *d_recs2, int nframes2, const int *d_counts2, const int *d_offsets2, int stride2,
                             int max_pts, int mutual,
                             void *d_out,          /* npairs * max_pts records (576 B each), device */
                             int *d_out_counts,    /* npairs, device */
                             int *d_num_matched);  /* npairs, device, may be NULL */

/* Batches in flight (no reference counterpart: ExtractSift is synchronous, cudaSiftH.cu:72-144).  A context is one
 * in-order pipeline; with K > 1 it owns K child pipelines (own stream, counters, candidate lists, detection staging) and
 * misift_extract_batch_packed_async hands consecutive calls to consecutive pipelines, so the HBM-bound prefilter of one
 * batch runs beside the VALU-bound kernels of another and launch tails are filled (+8-9 % frames/s at K = 3-4 on 64 x
 * 1080p).  Contract with K > 1:
 *   - every call still starts behind whatever was enqueued on the context stream before it (a marker is recorded there);
 *   - its results are NOT ordered on the context stream: observe them with misift_ctx_record_batch (an event of the
 *     caller's behind the most recent batch), misift_ctx_wait_batch (a stream of the caller's waits for it),
 *     misift_gather_post (marks the most recent batch) or misift_ctx_sync;
 *   - the scratch arena and the output buffers of a call must stay untouched until that batch is done: rotate >= K sets.
 *   - misift_match_batch, misift_match_pairs_batch, misift_quantize_batch, misift_match_batch_i8,
 *     misift_match_pairs_batch_i8, misift_select_pairs_batch, misift_find_homography_batch,
 *     misift_improve_homography_batch,
 *     misift_find_fundamental_batch, misift_score_fundamental_batch, misift_improve_fundamental_batch,
 *     misift_recover_pose_batch, misift_recover_pose_planar_batch, misift_link_poses_batch, misift_match_guided_batch,
 *     misift_match_epipolar_batch, misift_link_tracks_batch, misift_export_tracks_batch,
 *     misift_triangulate_tracks_batch, misift_refine_cameras_batch and misift_merge_scenes_batch (which run on the
 *     context stream) on a batch's
 *     packed records: make the context stream wait for that batch first
 *     (misift_ctx_wait_batch(ctx, <the context's stream>), or an event from misift_ctx_record_batch).
 * K = 1 (default) is the plain in-order context.  Also MISIFT_BATCHES_IN_FLIGHT at context creation.  Changing K drains
 * the context. */
int misift_ctx_set_batches_in_flight(misift_ctx *ctx, int k);
int misift_ctx_get_batches_in_flight(misift_ctx *ctx);
int misift_ctx_wait_batch(misift_ctx *ctx, void *stream);
/* Record the caller's hipEvent_t (passed as void*) behind the most recent batch, on the stream that batch runs on; the
 * caller then queries / waits on the event as it likes.  Preferable to misift_ctx_wait_batch when many side streams would
 * oversubscribe the hardware queues (a waiting stream that shares a queue with a pipeline holds that pipeline up). */
int misift_ctx_record_batch(misift_ctx *ctx, void *hip_event);

/* ------------------------------------------------------------ multi-GPU
 * The reference is single-GPU (InitCuda picks ONE device, cudaSiftH.cu:19-37); BASELINE configs 4 and 5 shard
 * frames / matcher rows over the GPUs of a node.  One misift_ctx per device (one host thread or process each) and
 * one misift_comm per context; collectives run on RCCL over xGMI, bound at run time (no link dependency: a
 * single-GPU caller never loads RCCL).  Nothing here touches the extraction data path — frames shard
 * embarrassingly; the only exchanges are the gather of SiftData after compute (config 4) and the set-2 /
 * result all-gathers around the matcher sweep (config 5). */
typedef struct misift_comm misift_comm;
#define MISIFT_COMM_ID_BYTES 128
/* Rendezvous like ncclGetUniqueId / ncclCommInitRank: rank 0 makes the id, ships its 128 bytes to the other
 * ranks by any means (MPI, a file, torch.distributed's store), every rank then creates its communicator on its
 * context's device.  misift_comm_adopt wraps a caller-supplied ncclComm_t instead (not destroyed with the comm). */
int misift_comm_unique_id(void *id128);
int misift_comm_create(misift_ctx *ctx, int nranks, int rank, const void *id128, misift_comm **out);
int misift_comm_adopt(misift_ctx *ctx, void *nccl_comm, misift_comm **out);
/* HOST communicator: no device and no context — counts, packed records and the receive buffer are HOST memory and the
 * five primitives of the exchange are the caller's callbacks (return 0 on success; send / recv may only queue, group_end
 * completes everything queued since the last call).  misift_comm_barrier, misift_gather_post (ctx = NULL),
 * misift_gather_test and misift_gather_complete run the SAME code above the transport as on RCCL — count staging,
 * per-rank record counts and offsets, root placement, -1 frames, the collective MISIFT_ENOMEM decision — which is what
 * the CPU-only suite drives over torch.distributed / gloo (tests/test_dist_cpu.py); misift_match_sharded needs a
 * device communicator.  Not a performance path. */
typedef struct misift_host_transport {
  void *user;
  int (*allgather)(void *user, const void *send, void *recv, size_t bytes_per_rank);
  int (*send)(void *user, const void *buf, size_t bytes, int peer);
  int (*recv)(void *user, void *buf, size_t bytes, int peer);
  int (*group_end)(void *user);
} misift_host_transport;
int misift_comm_create_host(int nranks, int rank, const misift_host_transport *transport, misift_comm **out);
/* In-process LOOPBACK WORLD ("fake N ranks on one GPU").  The reference has no multi-device code at
 * all (cudaSiftH.cu:19-37 picks one device), so nothing in it corresponds to this; it exists so that every N > 1
 * branch behind misift_gather_* / misift_match_sharded runs on the hardware a developer has: N communicators, one host
 * thread each, normally N contexts of ONE device, exchanging through a shared rendezvous object with device-to-device
 * copies instead of RCCL.  Same entry points, same code above the transport; functional only, never a scaling number.
 * A rank that never makes the matching call makes its peers fail with an error after MISIFT_LOOPBACK_TIMEOUT_S (60)
 * seconds instead of hanging; mismatching message sizes between the two sides of a send/recv are an error. */
typedef struct misift_loopback_world misift_loopback_world;
int misift_loopback_world_create(int nranks, misift_loopback_world **out);
void misift_loopback_world_destroy(misift_loopback_world *world);    /* after all its communicators */
int misift_comm_create_loopback(misift_ctx *ctx, misift_loopback_world *world, int rank, misift_comm **out);
void misift_comm_destroy(misift_comm *comm);
int misift_comm_rank(const misift_comm *comm);
int misift_comm_size(const misift_comm *comm);
int misift_comm_barrier(misift_comm *comm);        /* all ranks have arrived (host-blocking) */

/* BASELINE config 4 — gather of SiftData on `root`, pipelined under the next batches' extraction.
 *   misift_gather_post      right after misift_extract_batch_packed_async: remembers that batch's device buffers
 *                           (d_counts[nframes], d_packed) in `slot` (0..MISIFT_GATHER_SLOTS-1) and marks the point on
 *                           the stream of `ctx` where they are complete; `ctx` is the context that extracted the batch —
 *                           the communicator's own or any other context of the same device (several contexts per GPU
 *                           keep several batches in flight).  Returns at once.
 *   misift_gather_complete  on the communicator's own high-priority stream: all-gather of the per-frame counts
 *                           (nframes ints per rank, the same nframes on every rank), then ONE point-to-point message
 *                           per sender carrying exactly its valid 576-byte records (xGMI is a full mesh: 7 senders use
 *                           7 distinct links into the root).  h_all_counts[nranks*nframes] (host, every rank; -1 = that
 *                           frame's candidate list overflowed, no records); on the root the records of rank r land at
 *                           d_recv + h_rank_offsets[r] records (h_rank_offsets: nranks+1 entries, host, optional).
 *                           capacity_records = room at d_recv on the root, in records; pass the SAME value on every
 *                           rank: all ranks see all counts, so all of them return MISIFT_ENOMEM without exchanging
 *                           anything when the records do not fit (no rank is left waiting for a message).
 *                           Blocks the host until the transfer is done: the slot's buffers may be reused. */
#define MISIFT_GATHER_SLOTS 8
int misift_gather_post(misift_ctx *ctx, misift_comm *comm, int slot, const int *d_counts, int nframes,
                       const void *d_packed);
int misift_gather_complete(misift_comm *comm, int slot, int root, int *h_all_counts, void *d_recv,
                           size_t capacity_records, size_t *h_rank_offsets);
/* Non-blocking: *ready = 1 once the batch posted in `slot` has finished on the GPU (misift_gather_complete then only
 * waits for the exchange itself), 0 while its kernels are still running.  Lets a caller poll instead of parking a
 * thread in misift_gather_complete. */
int misift_gather_test(misift_comm *comm, int slot, int *ready);
/* Payload bytes this rank has received / sent over the links since the communicator was created (either may be NULL). */
int misift_comm_wire_bytes(misift_comm *comm, unsigned long long *received, unsigned long long *sent);

/* BASELINE config 5 — MatchSiftData (matching.cu:1090-1206) with set 1 split into row blocks, one per rank.
 * d_rows1: this rank's row block (row_count records, updated in place like misift_match); d_shard2: this rank's
 * shard of set 2 (shard_count records; row_count and shard_count must be equal on all ranks — pad the last block).
 * Steps: the shard is packed into MATCH COLUMNS — what the sweep reads of a record and nothing else:
 * MISIFT_MATCH_COLUMN_BYTES = 528 = descriptor[128], xpos, ypos, 2 reserved words (r04: 8 % less on the wire than the
 * 576-byte records r03 shipped) — and all-gathered into d_set2_all (nranks*shard_count columns, rank order; a buffer
 * sized for that many RECORDS is more than enough), then the fp32-MFMA sweep of the rank's rows over all of it, then
 * the all-gather of the 12-byte results {float score, float ambiguity, int match} of every row into d_results_all
 * (nranks*row_count entries, may be NULL).  Match indices refer to the gathered set 2.  Returns with everything in
 * place (matching.cu:1191).
 * Aliasing: d_shard2 must NOT overlap d_set2_all (the shard is re-packed into it; MISIFT_EINVAL otherwise — also with
 * one rank), and after the call d_set2_all holds 528-byte match columns, not SiftPoint records: look matched records
 * up in your own copy of set 2. */
#define MISIFT_MATCH_COLUMN_BYTES 528
int misift_match_sharded(misift_ctx *ctx, misift_comm *comm, void *d_rows1, int row_count, const void *d_shard2,
                         int shard_count, void *d_set2_all, void *d_results_all);

/* FindHomography (matching.cu:1000-1087): RANSAC over stored matches. */
int misift_find_homography(misift_ctx *ctx, const void *d_pts, int npts, float *homography9,
                           int *num_matches, int num_loops, float min_score,
                           float max_ambiguity, float thresh);

/* ImproveHomography (geomFuncs.cpp:6-72 — a host function over SiftData.h_data in the reference) on device-resident
 * records: num_loops rounds of least squares over the matches that pass the gates and currently reproject within
 * `thresh`, then match_error of every record is written (device) and *num_fit = records within thresh.
 * homography9: in = start (e.g. from misift_find_homography), out = refined, [8] = 1.  Sums in the reference's order:
 * bit-identical to the reference's result. */
int misift_improve_homography(misift_ctx *ctx, void *d_pts, int npts, float *homography9, int num_loops,
                              float min_score, float max_ambiguity, float thresh, int *num_fit);
/* Batched homography estimation (no reference counterpart; the C++ drop-in headers, cudaSift.h, do not change): entry i
 * works on frame frames[i] of a device-resident record batch and writes result slot i, stream-ordered on the context
 * stream, with no host synchronisation and no host read of the counts.  Together with misift_extract_batch_packed_async
 * and misift_match_batch a whole batch runs extract -> match -> find -> improve with no host read in between.
 * Frame f: its records start at d_recs + d_offsets[f] (d_offsets NULL: at f * stride records) and it holds
 * max(d_counts[f], 0) of them — the layout of misift_match_batch (set 1 of a match batch, match fields filled in).
 *   - find: d_homography[9i..9i+8] and d_num_matches[i] are bit-identical to srand(seeds[i]) followed by
 *     misift_find_homography on that frame alone (and to orc_find_homography after the same srand).  Each entry draws
 *     its samples on the device from its own seed (glibc's rand() restated); the process's rand() state is neither read
 *     nor changed.  Fewer than 8 records (count -1 included) or fewer than 8 valid points: identity H and 0.  Nothing is
 *     written into d_recs.
 *   - max_pts bounds the records of a frame, as in the extraction calls; temp memory is sized from nsel, max_pts and
 *     num_loops (rounded up to 16) only.  A frame whose device count exceeds max_pts is neither truncated nor read: it
 *     gets d_num_matches[i] = -1 and the identity H.
 *   - improve: d_homography (in: the start, e.g. find's result; out: the refined H, [8] = 1), d_num_fit[i] and the
 *     match_error of every record of the frame are bit-identical to misift_improve_homography(frame start,
 *     max(count, 0), H_i, ...); H_i is divided by H_i[8] on the device, and a frame with no records gets the zeroed
 *     solution when num_loops >= 1 (the Cholesky factorisation fails).  Only match_error is written.
 *   - The calls return before the GPU work is done.  `frames` and `seeds` (nsel entries each) are host memory the library
 *     copies: the caller may reuse them at once.
 *   - nsel < 0, a frame index outside [0, nframes), a repeated frame, a NULL output, num_loops < 1 (find) or < 0
 *     (improve), max_pts < 1: MISIFT_EINVAL, before anything is enqueued.  nsel == 0: nothing happens.
 *   - Find: four launches whatever nsel (gather + device draw, solve, count, pick); improve: one.
 *   - Directly behind misift_extract_batch_packed_async / misift_match_batch on the same context (K = 1) no
 *     synchronisation is needed.  With K > 1 batches in flight the extraction does not run on the context stream: order
 *     the call behind it with misift_ctx_wait_batch / misift_ctx_record_batch (see below). */
int misift_find_homography_batch(misift_ctx *ctx, int nsel, const int *frames, const unsigned *seeds,
                                 const void *d_recs, int nframes, const int *d_counts, const int *d_offsets,
                                 int stride, int max_pts, int num_loops, float min_score, float max_ambiguity,
                                 float thresh, float *d_homography /* nsel x 9 */, int *d_num_matches /* nsel */);
int misift_improve_homography_batch(misift_ctx *ctx, int nsel, const int *frames,
                                    void *d_recs, int nframes, const int *d_counts, const int *d_offsets, int stride,
                                    int num_loops, float min_score, float max_ambiguity, float thresh,
                                    float *d_homography /* in/out, nsel x 9 */, int *d_num_fit /* nsel */);
/* Batched fundamental-matrix estimation (no reference counterpart: the reference's only geometric model is the
 * homography, which fits a plane or a pure rotation; the C++ drop-in headers, cudaSift.h, do not change): the epipolar
 * counterpart of the two calls above, for general moving-camera scenes.  Frames, layouts (d_offsets or stride, count -1 =
 * no records), the host lists `frames` and `seeds` the library copies, stream order on the context stream with no host
 * synchronisation and no host read of the counts: as misift_find_homography_batch / misift_improve_homography_batch.
 * Convention: (x2, y2, 1) . F . (x1, y1, 1)^T = 0 with (x1, y1) = xpos, ypos and (x2, y2) = match_xpos, match_ypos of a
 * record; F is row-major in 9 floats.  All arithmetic is fp32 with every operation rounded (+ - * /, sqrtf, fabsf; no
 * fused multiply-add), so a restatement in numpy float32 reproduces every output bit.
 *   find, entry i with frame f = frames[i] and n = d_counts[f]:
 *   - A record is valid iff score > min_score && ambiguity < max_ambiguity (the gate of matching.cu:1035); the valid
 *     records keep index order.  n > max_pts: F = nine zeros and d_num_inliers[i] = -1, nothing of the frame is read.
 *     n < 8 (count -1 included) or fewer than 8 valid records: nine zeros and 0.  Nothing in d_recs is written.
 *   - Hypothesis h < num_loops (exactly num_loops hypotheses; temp memory rounds it up to 16) takes 8 distinct positions
 *     in the valid list from glibc's rand() restated on the device, seeded with seeds[i], the hypotheses drawing one
 *     after another from the one stream: p[0..7] = rand() % num_valid first, then for k = 1..7 in turn p[k] is redrawn
 *     while it equals some p[j], j < k.  The process's rand() state is neither read nor changed.
 *   - Normalisation per sample, for each of the two point sets: centroid = the sum in sample order times 0.125f,
 *     d = the sum in sample order of sqrtf(dx*dx + dy*dy), s = 11.3137085f / d, coordinates (x - cx) * s.
 *   - Solve: row k of the 8x9 system is (u2 u1, u2 v1, u2, v2 u1, v2 v1, v2, u1, v1, 1).  Gaussian elimination with
 *     complete pivoting: at step k the pivot is the entry of rows k..7 x columns k..8 with the largest fabsf, searched
 *     row-major with a strict '>' (the first maximum wins, a NaN never wins); rows and columns are swapped, row r > k
 *     becomes row r - (A[r][k] / pivot) * row k.  The remaining free column gets 1; back-substitution
 *     z[k] = -(sum over c > k, ascending, of A[k][c] * z[c]) / A[k][k]; the column permutation undone gives Fn, and
 *     F = T2^T . Fn . T1 with T = [s 0 -s*cx; 0 s -s*cy; 0 0 1], stored as computed: no rescaling, no rank-2 projection.
 *     A hypothesis is invalid iff a pivot is 0 or non-finite, or an entry of F is non-finite: its F is nine zeros and
 *     its count 0.
 *   - Count, over the valid records only: with a = F (x1, y1, 1)^T, b = F^T (x2, y2, 1)^T, e = x2*a0 + y2*a1 + a2 and
 *     den = a0*a0 + a1*a1 + b0*b0 + b1*b1, each summed left to right, a record is an inlier iff
 *     e*e < (thresh*thresh) * den: the squared Sampson distance against thresh^2, without the division.  A comparison
 *     with a NaN is false.
 *   - Pick: the largest count at the smallest hypothesis index; its F and count are d_fundamental[9i..9i+8] and
 *     d_num_inliers[i].  When every count is 0 that is hypothesis 0's F (zeros if it is invalid).
 *   - Four launches whatever nsel (gather + device draw, solve, count, pick); temp memory is sized from nsel, max_pts and
 *     num_loops (rounded up to 16) only.
 *   score, entry i: for EVERY record r < max(n, 0) of the frame, match_error = sqrtf((e*e) / den) under
 *   d_fundamental[9i..9i+8], +inf where den > 0 is false, and the quiet NaN 0x7fc00000 where that square root is a NaN
 *   (e*e NaN, or inf / inf: the sign and payload of a computed NaN are the processor's choice, so none is stored);
 *   d_num_fit[i] = the records that pass the gate above and the inlier test.  Only match_error is written.  One launch
 *   whatever nsel; an F of nine zeros gives +inf everywhere and 0.
 *   The rows of misift_match_pairs_batch(_i8) scored this way (frame i = pair i, d_offsets NULL, stride = max_pts,
 *   counts = d_out_counts) feed misift_link_tracks_batch through its max_error argument.
 *   - nsel < 0, a frame index outside [0, nframes), a repeated frame, a NULL ctx, records, counts or output pointer,
 *     max_pts < 1 or num_loops < 1 (find), thresh NaN or <= 0, d_offsets NULL with a negative stride: MISIFT_EINVAL,
 *     before anything is enqueued.  nsel == 0: nothing happens.
 *   - The calls return before the GPU work is done.  Ordering behind batches in flight (K > 1): as
 *     misift_find_homography_batch.
 *   - Least-squares refinement over the inliers: misift_improve_fundamental_batch, below; the relative pose of a pair
 *     from its F: misift_recover_pose_batch, below.  Out of scope: rank-2 enforcement. */
int misift_find_fundamental_batch(misift_ctx *ctx, int nsel, const int *frames, const unsigned *seeds,
                                  const void *d_recs, int nframes, const int *d_counts, const int *d_offsets,
                                  int stride, int max_pts, int num_loops, float min_score, float max_ambiguity,
                                  float thresh, float *d_fundamental /* nsel x 9, row-major */,
                                  int *d_num_inliers /* nsel */);
int misift_score_fundamental_batch(misift_ctx *ctx, int nsel, const int *frames,
                                   void *d_recs, int nframes, const int *d_counts, const int *d_offsets, int stride,
                                   float min_score, float max_ambiguity, float thresh,
                                   const float *d_fundamental /* nsel x 9 */, int *d_num_fit /* nsel */);
/* Refinement of batch fundamental matrices over their inliers (no reference counterpart): the epipolar counterpart of
 * misift_improve_homography_batch.  Entry i refits d_fundamental[9i..9i+8] up to num_loops times over the records of
 * frame frames[i] that pass the gate and currently lie within thresh, keeps a refit only if it loses no inlier, and then
 * writes match_error of every record under the result.  In the chain: find -> improve -> misift_match_epipolar_batch ->
 * improve (num_loops 0 or more) -> link.  Exactly as in misift_score_fundamental_batch: frames, layouts and count -1, the
 * copied host list `frames` with no frame repeated, stream order on the context stream with no host synchronisation and
 * no host read, ordering behind batches in flight, the convention (x2, y2, 1) . F . (x1, y1, 1)^T = 0, the gate
 * score > min_score && ambiguity < max_ambiguity, and the arithmetic rules: fp32, every operation rounded, only
 * + - * /, sqrtf and fabsf, no contraction, a comparison with a NaN is false.  No max_pts, no temp memory, one launch
 * whatever nsel.  Only match_error, d_fundamental, d_num_fit and d_num_rounds are written.
 *   Entry i has frame f and n = max(d_counts[f], 0) records.
 *   - The sum of the call.  Every floating-point sum of a quantity v over a record set S within [0, n) is taken in this
 *     order and no other: p[t], t < 256, starts at +0.0f and adds v(r) for the members r of S with r = t (mod 256), in
 *     ascending r (records that are no members are skipped, they do not add zero); then for off = 128, 64, ..., 1:
 *     p[t] = p[t] + p[t + off] for every t < off; the sum is p[0].
 *   - Setup.  F = d_fundamental[9i..9i+8] as given, all nine entries.  With G the records that pass the gate, inl(F) = the
 *     records of G with e*e < (thresh*thresh) * den (the inlier test of find, thresh*thresh rounded once on the host);
 *     c = |inl(F)|, rounds = 0.
 *   - Round, at most num_loops times:
 *     1. S = inl(F).  c < 8: stop.
 *     2. Normalise each of the two point sets over S: cx = SUM(x) / (float)c and cy likewise,
 *        d = SUM(sqrtf(dx*dx + dy*dy)) with dx = x - cx and dy = y - cy, s = ((float)c * 1.41421354f) / d, coordinates
 *        (x - cx) * s.
 *     3. Moments.  With a = (u2 u1, u2 v1, u2, v2 u1, v2 v1, v2, u1, v1, 1) the row of a record as in find:
 *        M[r][c'] = SUM(a[r] * a[c']) for r <= c' (45 sums), M[c'][r] = M[r][c'].
 *     4. Solve.  Gaussian elimination with complete pivoting on the 9x9 M, eight steps, by the rules of find's solve: at
 *        step k the pivot is the entry of rows k..8 x columns k..8 with the largest fabsf, searched row-major with a
 *        strict '>' (the first maximum wins, a NaN never wins); rows and columns are swapped, row r > k becomes
 *        row r - (A[r][k] / pivot) * row k.  The remaining free column gets 1; back-substitution of rows 7..0,
 *        z[k] = -(sum over c > k, ascending, of A[k][c] * z[c]) / A[k][k]; the column permutation undone gives Fn, and
 *        F' = T2^T . Fn . T1 with the expressions of find.  A pivot that is 0 or non-finite, or a non-finite entry of
 *        F': stop, F is kept.  For a symmetric positive semi-definite M this is the algebraic least squares
 *        min z^T M z with one component of z fixed to 1, and the pivoting leaves the best-determined component for
 *        that role.
 *     5. Accept.  c' = |inl(F')|.  c' >= c: F = F', c = c', rounds += 1.  Otherwise stop, F is kept.
 *   - End.  For EVERY record r < n, match_error under the final F as misift_score_fundamental_batch writes it (+inf
 *     where den > 0 is false, the quiet NaN 0x7fc00000 for a NaN).  d_fundamental[9i..9i+8] = F, d_num_fit[i] = c,
 *     d_num_rounds[i] = rounds (d_num_rounds may be NULL).
 *   - Consequences.  num_loops = 0 is misift_score_fundamental_batch, byte for byte.  Whatever num_loops is, the records
 *     and d_num_fit equal what misift_score_fundamental_batch writes under the returned F.  d_num_fit is never below
 *     the count of the start F.  An F of nine zeros, a frame with fewer than 8 inliers and a frame of count -1 leave F
 *     as it was.
 *   - NULL ctx, nsel < 0, a frame index outside [0, nframes), a repeated frame, NULL records, counts, d_fundamental or
 *     d_num_fit, num_loops < 0, thresh NaN or <= 0, d_offsets NULL with a negative stride: MISIFT_EINVAL, before
 *     anything is enqueued.  nsel == 0: nothing happens.
 *   - Out of scope: rank-2 enforcement, a geometric (Sampson) cost. */
int misift_improve_fundamental_batch(misift_ctx *ctx, int nsel, const int *frames,
                                     void *d_recs, int nframes, const int *d_counts, const int *d_offsets, int stride,
                                     int num_loops, float min_score, float max_ambiguity, float thresh,
                                     float *d_fundamental /* in/out, nsel x 9, row-major */,
                                     int *d_num_fit /* nsel */, int *d_num_rounds /* nsel, may be NULL */);
/* Relative camera pose per pair from batch fundamental matrices (no reference counterpart): the pose counterpart of
 * misift_score_fundamental_batch.  Entry i turns d_fundamental[9i..9i+8] and the two cameras' intrinsics into the
 * essential matrix, takes its four (R, t) decompositions, lets the inliers of frame frames[i] under F vote for the one
 * that puts them in front of both cameras, and triangulates every record of the frame under the winner.  In the chain:
 * find -> improve -> misift_match_epipolar_batch -> improve -> recover_pose -> link.  Exactly as in
 * misift_score_fundamental_batch / misift_improve_fundamental_batch: frames, layouts and count -1, the copied host lists
 * (`frames`, and `intrinsics` with it) with no frame repeated, stream order on the context stream with no host
 * synchronisation and no host read, ordering behind batches in flight, the convention
 * (x2, y2, 1) . F . (x1, y1, 1)^T = 0, the gate score > min_score && ambiguity < max_ambiguity and the inlier test
 * e*e < (thresh*thresh) * den, the arithmetic rules (fp32, every operation rounded, only + - * /, sqrtf and fabsf, no
 * contraction, a comparison with a NaN is false) and the MISIFT_EINVAL list, with d_pose and d_num_front the outputs that
 * must not be NULL.  Two more cases are MISIFT_EINVAL, checked on the host before anything is enqueued: a NULL
 * `intrinsics`, and an fx or fy that is not finite and > 0 or a cx or cy that is not finite.  d_recs is not written.  One
 * launch whatever nsel, no temp memory.  The pose convention is X2 = R . X1 + t with |t| = 1: the scale of the scene is
 * not observable from two views.
 *   intrinsics[8i..8i+7] = fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2: K1 of the image that holds (x1, y1), K2 of the other.
 *   Entry i has frame f and n = max(d_counts[f], 0) records.  Every sum of products is taken left to right as written.
 *   1. E = K2^T . F . K1.  G[r][0] = F[r][0]*fx1, G[r][1] = F[r][1]*fy1, G[r][2] = (F[r][0]*cx1 + F[r][1]*cy1) + F[r][2];
 *      E[0][c] = fx2*G[0][c], E[1][c] = fy2*G[1][c], E[2][c] = (cx2*G[0][c] + cy2*G[1][c]) + G[2][c].  m = the largest
 *      fabsf of E.  The entry is INVALID if an entry of E is non-finite or m is 0.  Otherwise A = E / m entry by entry, and
 *      V = I.
 *   2. Six sweeps of one-sided Jacobi over the column pairs (0,1), (0,2), (1,2) in that order.  For a pair (p, q):
 *      alpha = A.p . A.p, beta = A.q . A.q, gamma = A.p . A.q (three-term sums over the rows).  gamma == 0: no rotation.
 *      Otherwise zeta = (beta - alpha) / (2*gamma), tau = 1 / (fabsf(zeta) + sqrtf(1 + zeta*zeta)), negated when
 *      zeta < 0, c = 1 / sqrtf(1 + tau*tau), s = c*tau; new column p = c * old p - s * old q, new column q =
 *      s * old p + c * old q, for A and V alike.  The count is fixed: there is no convergence test, every entry runs the
 *      same instructions.
 *   3. Bases.  w[j] = the squared norm of column j of A.  i1 = the index of the largest w, searched with a strict '>'
 *      (the first maximum wins); i2 = the larger of the other two (again the first wins).  The entry is INVALID unless
 *      w[i2] > 0.  u1 = A.i1 / sqrtf(w[i1]), u2 = A.i2 / sqrtf(w[i2]), u3 = u1 x u2; v1 = V.i1, v2 = V.i2, v3 = v1 x v2;
 *      every component of a cross product is (a*b) - (c*d).  The null direction is never taken from the near-zero column,
 *      and both bases are right-handed by construction.
 *   4. Hypotheses k = 0..3.  Ra[r][c] = (u2[r]*v1[c] - u1[r]*v2[c]) + u3[r]*v3[c], Rb[r][c] = (u1[r]*v2[c] -
 *      u2[r]*v1[c]) + u3[r]*v3[c]; R = Ra for k < 2, otherwise Rb; t = u3 for even k, -u3 for odd k.
 *   5. Vote, over the records that pass the gate and the inlier test under F as given (inl(F) of improve).  For such a
 *      record and a hypothesis: p1 = ((x1 - cx1) / fx1, (y1 - cy1) / fy1, 1) and p2 likewise from K2; a = R . p1 (each
 *      row a three-term sum), n = a x p2, den = n . n, n1 = (p2 x t) . n, n2 = (a x t) . n.  The record is IN FRONT iff
 *      den > 0 && n1 > 0 && n2 > 0.  n1 / den and n2 / den are the least-squares depths z1, z2 of z1 a - z2 p2 = -t; the
 *      cross-product form keeps its digits at the parallax of neighbouring video frames, where aa*bb - ab*ab cancels.
 *      votes[k] = the records in front under hypothesis k.
 *   6. Pick: the largest vote at the smallest k.  d_pose[12i..12i+11] = its R, row-major, then its t; d_num_front[i] =
 *      its vote; d_votes[4i..4i+3] = the four votes (d_votes may be NULL).  An INVALID entry gives twelve zeros, 0 and
 *      four zeros.  A valid F with no inlier (count -1 and count 0 included) gives hypothesis 0 and 0.
 *   7. d_xyz, when not NULL: for EVERY record r < n of the frame, the four floats at its global record index (the index it
 *      has in d_recs) are (z1*p1x, z1*p1y, z1, z2) under the picked pose: the point in the frame of camera 1, and its
 *      depth in camera 2.  The four are the quiet NaN 0x7fc00000 where den > 0 is false and for every record of an INVALID
 *      entry; a single result that is a NaN is stored as 0x7fc00000 (see match_error above).  Negative depths are stored
 *      as computed.  Records of frames that are not selected are not touched. */
int misift_recover_pose_batch(misift_ctx *ctx, int nsel, const int *frames,
                              const float *intrinsics /* host, nsel x 8: fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2, copied */,
                              const void *d_recs, int nframes, const int *d_counts, const int *d_offsets, int stride,
                              float min_score, float max_ambiguity, float thresh,
                              const float *d_fundamental /* nsel x 9 */,
                              float *d_pose      /* nsel x 12: R row-major, then t */,
                              int   *d_num_front /* nsel */,
                              int   *d_votes     /* nsel x 4, may be NULL */,
                              float *d_xyz       /* 4 floats per record, indexed like d_recs, may be NULL */);
/* Relative camera pose per pair from batch homographies, for planar and rotation-only pairs (no reference counterpart).
 * A fundamental matrix is degenerate where every match lies on one plane (the 8-point solve fits a one-parameter family
 * and misift_recover_pose_batch decomposes an arbitrary member into a confident wrong pose) and undefined where the
 * camera only rotates.  This call sits behind misift_recover_pose_batch in the chain,
 *   ... find_fundamental -> improve_fundamental -> recover_pose -> recover_pose_planar -> link_poses ...,
 * with d_homography from misift_find_homography_batch / misift_improve_homography_batch over the same frames, and
 * OVERWRITES d_pose, d_num_front, d_votes and the frame's d_xyz rows of exactly those entries it judges planar (model 1)
 * or rotation-only (model 2); an entry it judges general (model 0) or cannot decompose (model -1) keeps what
 * misift_recover_pose_batch wrote: apart from d_model and d_hf_counts, nothing of such an entry is written.  With
 * d_fundamental NULL every entry with enough H-inliers is a candidate: the stand-alone use behind the homography calls.
 * Exactly as in misift_recover_pose_batch: frames, layouts and count -1, the copied host lists (`frames`, and
 * `intrinsics` with it, intrinsics[8i..8i+7] = fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2) with no frame repeated, stream order on
 * the context stream with no host synchronisation and no host read, ordering behind batches in flight, the pose
 * convention X2 = R . X1 + t with |t| = 1, the gate score > min_score && ambiguity < max_ambiguity, the arithmetic rules
 * (fp32, every operation rounded, only + - * /, sqrtf and fabsf, no contraction, a comparison with a NaN is false, a
 * stored NaN is 0x7fc00000) and its MISIFT_EINVAL list, with d_homography, d_model, d_hf_counts, d_pose and d_num_front the
 * pointers that must not be NULL (d_fundamental may be).  Five more cases are MISIFT_EINVAL, checked on the host before
 * anything is enqueued: thresh_h or thresh_f NaN or <= 0, planar_ratio NaN or < 0, min_inliers < 4, min_baseline NaN or
 * < 0.  d_recs is not written.  One launch whatever nsel, no temp memory.
 *   d_homography[9i..9i+8] = H, row-major, set-1 pixel positions to set-2 pixel positions, all nine entries used as
 *   given.  Entry i has frame f and n = max(d_counts[f], 0) records.  A sum written a*b + c*d + e*f is taken left to
 *   right, (a*b + c*d) + e*f; every other association is written out.  A cross product's component is (a*b) - (c*d).
 *   1. Count, over the records that pass the gate.  deno = (h6*x1 + h7*y1) + h8, nomx = (h0*x1 + h1*y1) + h2, nomy =
 *      (h3*x1 + h4*y1) + h5, errx = x2*deno - nomx, erry = y2*deno - nomy; the record is an H-INLIER iff
 *      errx*errx + erry*erry < (thresh_h*thresh_h) * (deno*deno).  nH = the H-inliers.  These are plain rounded products:
 *      the round-toward-zero products of the reference's homography search (misift_find_homography_batch) are not
 *      restated here, so a borderline record may count differently from that call's own count.  nF = |inl(F)| of
 *      misift_improve_fundamental_batch under d_fundamental[9i..9i+8] at thresh_f, 0 when d_fundamental is NULL.
 *      d_hf_counts[2i] = nH, d_hf_counts[2i+1] = nF, always.
 *   2. Decide.  d_model[i] = 0 if nH < min_inliers, or if d_fundamental is given and (float)nH >= planar_ratio *
 *      (float)nF is false.  planar_ratio 0.8 is recommended (COLMAP's max_H_inlier_ratio).  Nothing else of a model-0
 *      entry is written.
 *   3. Normalise.  A = K2^-1 . H . K1: G[r][0] = H[r][0]*fx1, G[r][1] = H[r][1]*fy1, G[r][2] = (H[r][0]*cx1 +
 *      H[r][1]*cy1) + H[r][2]; A[0][c] = (G[0][c] - cx2*G[2][c]) / fx2, A[1][c] = (G[1][c] - cy2*G[2][c]) / fy2, A[2][c] =
 *      G[2][c].  m = the largest fabsf of A.  The entry is INVALID (d_model[i] = -1, nothing else written) if an entry of
 *      A is non-finite or m is 0.  A = A / m entry by entry.  det = (A00*(A11*A22 - A12*A21) - A01*(A10*A22 - A12*A20)) +
 *      A02*(A10*A21 - A11*A20).  If det < 0 every entry of A is negated and det is computed again; INVALID if det > 0 is
 *      then false.  (H and -H are one homography; the one with the positive determinant keeps the camera on one side of
 *      the plane it sees.)
 *   4. Jacobi.  B = A, V = I; six sweeps of step 2 of misift_recover_pose_batch over the column pairs (0,1), (0,2),
 *      (1,2), applied to B and V alike.  w[j] = the squared norm of column j of B.  hi = the index of the largest w,
 *      searched with a strict '>' (the first maximum wins); mid = the larger of the other two (again the first wins);
 *      lo = the third.  INVALID unless w[lo] > 0.  s1 = w[hi] / w[mid], s3 = w[lo] / w[mid].
 *   5. Rotation-only.  b = sqrtf(s1) - sqrtf(s3): |t| over the distance of the plane.  If b > min_baseline is false,
 *      d_model[i] = 2: with u_j = B.j / sqrtf(w[j]), R[r][c] = (u_0[r]*V[c][0] + u_1[r]*V[c][1]) + u_2[r]*V[c][2], and
 *      t = 0.  d_pose = R then three zeros, d_pose_alt the same twelve floats, d_num_front[i] = 0 (so
 *      misift_link_poses_batch skips the pair), d_votes four zeros, d_plane four zeros, and every d_xyz row of the frame
 *      four quiet NaNs.  (A fit of 400 matches with 0.5 px noise under a pure rotation leaves b near 1e-3; min_baseline
 *      0.02 separates that from a baseline of a fiftieth of the plane's distance.)
 *   6. Planar, d_model[i] = 1.  Hn = A (after the sign, before the sweeps) / sqrtf(w[mid]).  v1, v2, v3 = the columns
 *      hi, mid, lo of V.  a = sqrtf(1 - s3), c = sqrtf(s1 - 1), dd = sqrtf(s1 - s3); ua = (a*v1 + c*v3) / dd and ub =
 *      (a*v1 - c*v3) / dd, component by component.  For u = ua and u = ub: N = v2 x u; p = Hn . v2 and q = Hn . u (each
 *      row a three-term sum); s = p x q; R[r][c] = (p[r]*v2[c] + q[r]*u[c]) + s[r]*N[c]; T[r] = ((Hn[r][0] - R[r][0])*N[0]
 *      + (Hn[r][1] - R[r][1])*N[1]) + (Hn[r][2] - R[r][2])*N[2]; |T| = sqrtf(T.T); t = T / |T|, d = 1 / |T|.  INVALID if a
 *      |T| is not finite and > 0.  The plane is N . X1 = d in the frame of camera 1, d in units of |t|.  The hypotheses
 *      are k = 0: (Ra, ta, Na, da), 1: (Ra, -ta, -Na, da), 2: (Rb, tb, Nb, db), 3: (Rb, -tb, -Nb, db).
 *   7. Vote, over the records that pass the gate (H-inliers or not).  For k = 0 and k = 2, F_k = K2^-T . [t]x . R .
 *      K1^-1: E[0][c] = t1*R[2][c] - t2*R[1][c], E[1][c] = t2*R[0][c] - t0*R[2][c], E[2][c] = t0*R[1][c] - t1*R[0][c];
 *      G[r][0] = E[r][0] / fx1, G[r][1] = E[r][1] / fy1, G[r][2] = (E[r][2] - G[r][0]*cx1) - G[r][1]*cy1; F[0][c] =
 *      G[0][c] / fx2, F[1][c] = G[1][c] / fy2, F[2][c] = (G[2][c] - cx2*F[0][c]) - cy2*F[1][c].  Under -t, F changes sign
 *      and the test does not, so k = 1 and 3 share F_0 and F_2.  A record counts for k iff e*e < (thresh_f*thresh_f) * den
 *      under F_k and it is IN FRONT under (R_k, t_k), both exactly as in misift_recover_pose_batch.  Records on the plane
 *      satisfy both rotations' epipolar geometry by construction and vote through their depths alone, which separates
 *      +-N; records off the plane separate Ra from Rb.  Pick: the largest vote at the smallest k.  The alternative: of
 *      the two hypotheses of the other rotation, the one with the larger vote (the smaller k on a tie).  The two-fold
 *      ambiguity of an exactly planar scene is real: no two-view test resolves it.  d_votes and d_pose_alt are how the
 *      caller sees it, and a third view is how it is resolved; this call does not do that.
 *   8. Outputs of a model-1 entry, as misift_recover_pose_batch writes them: d_pose[12i..12i+11] = R then t of the pick,
 *      d_num_front[i] = its vote, d_votes[4i..4i+3] = the four votes, d_xyz for EVERY record r < n of the frame under the
 *      pick (step 7 of that call, the entry valid); d_pose_alt[12i..12i+11] = R then t of the alternative; d_plane[4i..
 *      4i+3] = N then d of the pick.  d_votes, d_xyz, d_pose_alt and d_plane may each be NULL. */
int misift_recover_pose_planar_batch(misift_ctx *ctx, int nsel, const int *frames,
                                     const float *intrinsics /* host, nsel x 8, as misift_recover_pose_batch, copied */,
                                     const void *d_recs, int nframes, const int *d_counts, const int *d_offsets,
                                     int stride, float min_score, float max_ambiguity,
                                     float thresh_h, float thresh_f, float planar_ratio, int min_inliers,
                                     float min_baseline,
                                     const float *d_homography  /* nsel x 9, set-1 px -> set-2 px */,
                                     const float *d_fundamental /* nsel x 9, may be NULL */,
                                     int   *d_model      /* nsel: -1 invalid, 0 general (entry left alone), 1 planar,
                                                            2 rotation */,
                                     int   *d_hf_counts  /* nsel x 2: nH, nF */,
                                     float *d_pose       /* nsel x 12, written for model 1 and 2 only */,
                                     int   *d_num_front  /* nsel, likewise */,
                                     int   *d_votes      /* nsel x 4, likewise, may be NULL */,
                                     float *d_xyz        /* 4 floats per record, rows of model 1 and 2 entries only,
                                                            may be NULL */,
                                     float *d_pose_alt   /* nsel x 12, likewise, may be NULL */,
                                     float *d_plane      /* nsel x 4: N (camera 1) and d in units of |t|, likewise, may
                                                            be NULL */);
/* Homography-guided matching (no reference counterpart as an API: MatchAll, mainSift.cpp:95-147, does it as a host
 * diagnostic; the C++ drop-in headers, cudaSift.h, do not change): for each pair i = (f1, f2) = (pairs[2i], pairs[2i+1]),
 * every record of frame f1 of set 1 is matched only against the records of frame f2 of set 2 that lie within `radius`
 * of its projection through d_homography[9i..9i+8] (set-1 positions to set-2 positions; the layout of
 * misift_find_homography_batch's output when frames[i] is pair i's set-1 frame; all nine entries used as given),
 * stream-ordered on the context stream, with no host synchronisation and no host read of the counts.
 * Frames, pairs and layouts as in misift_match_batch: d_offsets or stride, count -1 = no records, a set-1 frame in at
 * most one pair, a set-2 frame in any number (keyframe mode), d_recs1 == d_recs2 allowed.  With n1 = max(count1[f1], 0)
 * and n2 = max(count2[f2], 0):
 *   - n1 > max_pts or n2 > max_pts: set 1 untouched, d_num_found[i] = -1.  n1 == 0 or n2 == 0: untouched, 0.
 *   - Otherwise every row (x, y) of set 1, in fp32 with every operation rounded (no contraction):
 *     den = H6*x + H7*y + H8, px = (H0*x + H1*y + H2) / den, py = (H3*x + H4*y + H5) / den; record j of set 2 is a
 *     candidate iff (px - x2)*(px - x2) + (py - y2)*(py - y2) < radius*radius (rounded to fp32 once).  A non-finite
 *     projection or position is never a candidate.  Scores are the matcher's k-ordered fmaf chain; the row gets the
 *     exact top-2 over its candidates as misift_match with match_full = 1, match_exact_top2 = 1 would give it (only
 *     scores > 0 count, match = the smallest frame-local index that attains the best score, -1 and score 0 when none
 *     does), whatever the options of the context.  d_num_found[i] = rows with match >= 0 (d_num_found may be NULL).
 *     radius = +inf with the identity H equals misift_match in that mode, byte for byte.
 *   - Only score, ambiguity, match, match_xpos and match_ypos of set-1 rows of some pair are written.
 *   - The call returns before the GPU work is done.  `pairs` (npairs x 2 ints) is host memory the library copies: the
 *     caller may reuse it at once.
 *   - npairs < 0, a frame index outside [0, nframes) of its set, a repeated set-1 frame, NULL records, counts or
 *     d_homography, radius NaN or <= 0, max_pts < 1: MISIFT_EINVAL, before anything is enqueued.  npairs == 0: nothing
 *     happens.
 *   - Two launches whatever npairs (bin set 2 into a cell grid, match); temp memory is sized from npairs, the distinct
 *     set-2 frames and max_pts only, and no descriptor dot product is computed for a non-candidate.
 *   - Directly behind misift_extract_batch_packed_async / misift_match_batch / misift_find_homography_batch on the same
 *     context (K = 1) no synchronisation is needed.  With K > 1 batches in flight the extraction does not run on the
 *     context stream: order the call behind it with misift_ctx_wait_batch / misift_ctx_record_batch (see below). */
int misift_match_guided_batch(misift_ctx *ctx, int npairs, const int *pairs,
                              void *d_recs1, int nframes1, const int *d_counts1, const int *d_offsets1, int stride1,
                              const void *d_recs2, int nframes2, const int *d_counts2, const int *d_offsets2, int stride2,
                              const float *d_homography /* npairs x 9, device */, float radius, int max_pts,
                              int *d_num_found /* npairs, device, may be NULL */);
/* Epipolar-guided matching (no reference counterpart; the C++ drop-in headers do not change): the moving-camera
 * counterpart of misift_match_guided_batch.  For each pair i, every record of frame f1 of set 1 is matched only against
 * the records of frame f2 of set 2 that lie within `radius` of its epipolar line under d_fundamental[9i..9i+8], in the
 * convention of misift_find_fundamental_batch, (x2, y2, 1) . F . (x1, y1, 1)^T = 0 (the layout of its output when
 * frames[i] is pair i's set-1 frame; all nine entries used as given).  In the chain: misift_match_batch ->
 * misift_find_fundamental_batch -> misift_match_epipolar_batch -> misift_score_fundamental_batch -> link -> export.
 * Everything not said here is the contract of misift_match_guided_batch, word for word: pairs and layouts, count -1,
 * a set-1 frame in at most one pair and a set-2 frame in any number, d_recs1 == d_recs2, max_pts (-1, untouched) and
 * empty sides (0, untouched), the five fields written, the copied `pairs`, the stream order with no host
 * synchronisation and no host read, the two launches (the same bin launch, then the epipolar match kernel), the temp
 * memory, the MISIFT_EINVAL list with d_fundamental in the place of d_homography, and npairs == 0.
 *   - The gate, for row (x, y) of set 1, in fp32 with every operation rounded (no contraction), sums left to right:
 *     a0 = F0*x + F1*y + F2, a1 = F3*x + F4*y + F5, a2 = F6*x + F7*y + F8, n2 = a0*a0 + a1*a1 (the `a` terms of the
 *     Sampson test); record j of set 2 at (x2, y2) is a candidate iff, with e = x2*a0 + y2*a1 + a2,
 *     e*e < (radius*radius) * n2: the squared point-to-line distance in image 2 against radius^2, without the division;
 *     radius*radius is rounded to fp32 once on the host.
 *   - A row whose a0, a1, a2 or n2 is non-finite (an overflowing n2 included) has no candidate.  Otherwise the
 *     comparison decides as written: a NaN comparison is false, n2 == 0 admits nothing, a right-hand side of +inf
 *     (radius = +inf, or an overflowing finite product) admits every record whose e*e is finite.  A set-2 record with a
 *     non-finite position is never a candidate.
 *   - The row gets the exact top-2 over its candidates (k-ordered fmaf chain; only scores > 0 count; match = the smallest
 *     frame-local index that attains the best score; a second copy of the best score is the runner-up); a row with no
 *     candidate gets match -1, score 0, ambiguity 0 and match positions 0; whatever the options of the context.
 *     radius = +inf with a finite non-zero F equals misift_match with match_full = 1, match_exact_top2 = 1, byte for byte.
 *   - The result is the gate's alone: the walk that finds the candidates (a band across the cell grid) is conservative
 *     and leaves no trace in the output. */
int misift_match_epipolar_batch(misift_ctx *ctx, int npairs, const int *pairs,
                                void *d_recs1, int nframes1, const int *d_counts1, const int *d_offsets1, int stride1,
                                const void *d_recs2, int nframes2, const int *d_counts2, const int *d_offsets2, int stride2,
                                const float *d_fundamental /* npairs x 9, row-major, device */, float radius, int max_pts,
                                int *d_num_found /* npairs, device, may be NULL */);

/* 8-bit descriptors (no reference counterpart; the C++ drop-in headers do not change): for every record r of every frame
 * of a device-resident batch (frames as in misift_match_batch: d_offsets or stride, max(d_counts[f], 0) records),
 * d_q[128 r + k] = (int8) clamp(rint(256 * data[k]), 0, 127), r being the record's global index — so d_q mirrors the
 * record index space and misift_match_batch_i8 takes the same counts, offsets and stride.  rint rounds half to even in
 * fp32 (256 * d is exact); NaN -> 0, +inf -> 127, negative values -> 0.  No other byte of d_q is written.
 *   - One launch, stream-ordered on the context stream, with no host read of the counts; the call returns before the
 *     GPU work is done.
 *   - NULL d_recs, d_counts or d_q, d_q not 16-byte aligned, nframes < 0, or d_offsets NULL with stride < 0:
 *     MISIFT_EINVAL, before anything is enqueued.  nframes == 0: nothing happens.
 *   - Directly behind misift_extract_batch_packed_async on the same context (K = 1) no synchronisation is needed; with
 *     K > 1 batches in flight order it with misift_ctx_wait_batch / misift_ctx_record_batch (see below). */
int misift_quantize_batch(misift_ctx *ctx, const void *d_recs, int nframes, const int *d_counts, const int *d_offsets,
                          int stride, int8_t *d_q /* 128 bytes per record, device, 16-byte aligned */);
/* Batched pair matching on 8-bit descriptors and the int8 matrix cores (no reference counterpart; opt-in: every other
 * call keeps its bits).  Pairs, frames, layouts, argument checks and stream semantics are those of misift_match_batch;
 * d_q1 / d_q2 are the 128-byte descriptors of the records of d_recs1 / d_recs2 at the same record indices (what
 * misift_quantize_batch writes).  The call reads only q and set 2's xpos / ypos.  For each row i of a pair with n1 > 0
 * and n2 > 0, against every column j of its set-2 frame (whatever match_full / match_exact_top2 say):
 *   - S_ij = sum_k q1[i][k] * q2[j][k], exact in int32; only S_ij > 0 counts.  best = the largest, m = the SMALLEST
 *     frame-local j that attains it, second = the largest over j != m (0 when there is none).
 *   - score = (float)best * 2^-16 (exact; 0 when no S_ij > 0), ambiguity = ((float)second * 2^-16) / (score + 1e-6f) in
 *     fp32, match = m or -1, match_xpos / match_ypos = xpos / ypos of set-2 record m, or 0.  For quantised unit
 *     descriptors score is a cosine on the scale of misift_match's, so the rows feed misift_find_homography_batch as
 *     they are.
 *   - Only those five fields of set-1 rows of some pair are written; a pair with an empty side stays untouched.
 *   - d_recs1 == d_recs2 and d_q1 == d_q2 are allowed.  A set-1 frame may appear in at most one pair, a set-2 frame in
 *     any number.  `pairs` is host memory the library copies.  The call returns before the GPU work is done.
 *   - npairs < 0, a frame index outside [0, nframes) of its set, a repeated set-1 frame, a NULL pointer, d_q1 or d_q2
 *     not 16-byte aligned: MISIFT_EINVAL, before anything is enqueued.  npairs == 0: nothing happens.
 *   - Three launches whatever npairs (plan, sweep, merge of chunked columns); temp memory is sized from npairs and the
 *     CU count only, never by max_pts.
 *   - Ordering behind misift_extract_batch_packed_async / misift_quantize_batch as for misift_match_batch. */
int misift_match_batch_i8(misift_ctx *ctx, int npairs, const int *pairs,
                          void *d_recs1, const int8_t *d_q1, int nframes1, const int *d_counts1, const int *d_offsets1,
                          int stride1,
                          const void *d_recs2, const int8_t *d_q2, int nframes2, const int *d_counts2,
                          const int *d_offsets2, int stride2);
/* Pair-indexed batch matching on 8-bit descriptors (no reference counterpart; opt-in: every other call keeps its bits):
 * misift_match_pairs_batch with the scores of misift_match_batch_i8.  Pairs, frames, layouts (d_offsets or stride),
 * count -1 = no records, the host `pairs` the library copies, stream order on the context stream with no host
 * synchronisation and no host read of the counts, and ordering behind batches in flight (K > 1): as
 * misift_match_pairs_batch.  d_q1 / d_q2 are the 128-byte descriptors of the records of d_recs1 / d_recs2 at the same
 * record indices (what misift_quantize_batch writes).  For pair i = (f1, f2), n1 = max(count1[f1], 0) and
 * n2 = max(count2[f2], 0).
 *   - A set-1 frame and a set-2 frame may appear in any number of pairs; (f, f), d_recs1 == d_recs2 and d_q1 == d_q2 are
 *     allowed.  Nothing in d_recs1, d_recs2, d_q1 or d_q2 is written.  The call reads only q, set 1's xpos / ypos and
 *     set 2's xpos / ypos.
 *   - n1 > max_pts or n2 > max_pts: d_out_counts[i] = -1 and d_num_matched[i] = -1; none of the pair's output bytes is
 *     written.  Otherwise d_out_counts[i] = n1, and output row r < n1 of pair i is the record d_out + (i * max_pts + r),
 *     of which exactly seven fields are written: xpos and ypos (set-1 record r's), and score, ambiguity, match,
 *     match_xpos, match_ypos, byte-identical to what misift_match_batch_i8 on that pair writes into set-1 record r:
 *     S_rj = sum_k q1[r][k] * q2[j][k], exact in int32, over every column j (whatever match_full / match_exact_top2
 *     say); only S > 0 counts; m = the smallest frame-local j of the largest S, second = the largest over j != m;
 *     score = (float)best * 2^-16, ambiguity = ((float)second * 2^-16) / (score + 1e-6f).  n2 == 0: every row is a
 *     no-match row (score 0, ambiguity 0, match -1, match_xpos 0, match_ypos 0).  Every other byte of d_out is untouched.
 *   - mutual = 1 (cross-check): a row r with forward match m >= 0 keeps it only if r is the best row of column m over
 *     all n1 rows — the largest S_rm > 0, the smallest row on a tie: the match misift_match_batch_i8 with the two sets
 *     swapped writes for set-2 record m; otherwise it becomes a no-match row.  mutual = 0: no filter.
 *   - d_num_matched (may be NULL): per pair, the output rows with match >= 0 after the filter.
 *   - The output is a batch the homography calls take as it is: frame i = pair i, d_offsets NULL, stride = max_pts,
 *     counts = d_out_counts (misift_find_homography_batch, misift_improve_homography_batch).
 *   - NULL ctx, npairs < 0, a frame index outside [0, nframes) of its set, a NULL records, q, counts, d_out or
 *     d_out_counts pointer, d_q1 or d_q2 not 16-byte aligned, max_pts < 1, mutual other than 0 or 1, d_out equal to
 *     d_recs1 or d_recs2, d_offsets NULL with a negative stride: MISIFT_EINVAL, before anything is enqueued.
 *     npairs == 0: MISIFT_OK, nothing happens.
 *   - The call returns before the GPU work is done.  Three launches and, with mutual, one memset, whatever npairs (plan,
 *     sweep, finalize); temp memory is sized from npairs, max_pts and the CU count only. */
int misift_match_pairs_batch_i8(misift_ctx *ctx, int npairs, const int *pairs,
                                const void *d_recs1, const int8_t *d_q1, int nframes1, const int *d_counts1,
                                const int *d_offsets1, int stride1,
                                const void *d_recs2, const int8_t *d_q2, int nframes2, const int *d_counts2,
                                const int *d_offsets2, int stride2,
                                int max_pts, int mutual,
                                void *d_out,          /* npairs * max_pts records (576 B each), device */
                                int *d_out_counts,    /* npairs, device */
                                int *d_num_matched);  /* npairs, device, may be NULL */

/* Preemptive matching (no reference counterpart; Wu, "Towards linear-time incremental structure from motion"): WHICH
 * frame pairs of an unordered batch are worth matching, decided on the device.  Only the `top` largest-scale features of
 * every frame are matched against those of every other frame on the int8 matrix cores, only a vote count per pair is
 * kept, and every frame proposes its k best partners.  The call fills the `pairs` array the pair matchers take, in place
 * of an exhaustive list.  One record batch as in misift_link_tracks_batch (d_recs, nframes, d_counts, d_offsets or
 * stride; a count of -1 means no records: n = max(count, 0)); d_q are its 128-byte descriptors from
 * misift_quantize_batch.  Of the records only `scale` is read.
 *   1. Features.  The key of record r is the bit pattern of scale if scale > 0, else 0 (a NaN compares false: 0; +inf is
 *      the largest key).  The chosen records of frame f are the h(f) = min(n, top) records with the largest keys, ordered
 *      by key descending, then index ascending.  d_sel[f * top + i] = the frame-local index of the i-th, or -1 for
 *      i >= h(f); d_sel_counts[f] = h(f).
 *   2. Votes, for every unordered pair a < b, on the chosen descriptors qa (rows) and qb (columns) in the order of d_sel:
 *      S_ij = sum_k qa[i][k] * qb[j][k], exact in int32.  Row i: best = the largest S_ij > 0, m = the smallest j that
 *      attains it, second = the largest S_ij over j != m, or 0 (the rule of misift_match_batch_i8).  Column m's best row
 *      is the row with the largest S_im > 0, the smallest row on a tie (the mutual rule of misift_match_pairs_batch_i8).
 *      Row i votes iff m >= 0, row i is column m's best row, score = (float)best * 2^-16 > min_score, and
 *      ((float)second * 2^-16) / (score + 1e-6f) < max_ambiguity in fp32.  V[a][b] = V[b][a] = the voting rows,
 *      V[f][f] = 0: the rows misift_match_pairs_batch_i8(mutual = 1) on the two gathered subsets would write and the gate
 *      of misift_link_tracks_batch with max_error = +inf would accept.  d_votes (nframes x nframes) is fully written.
 *   3. Pairs.  The neighbours of f are the g != f with V[f][g] >= min_votes, ordered by V descending, then g ascending;
 *      the first k are taken.  Pair (a, b), a < b, is selected iff b is a neighbour taken by a or a one taken by b.  With
 *      P selected pairs, for i < min(P, max_pairs) in ascending (a, b) order: d_pairs[2i], d_pairs[2i + 1] = (a, b) and
 *      d_pair_votes[i] = V[a][b].  d_summary (8 ints): [0] P, [1] pairs written, [2] frames with at least one record and
 *      no neighbour, [3] frames with more than `top` records, [4] the largest V, [5] = [6] = [7] = 0.
 *   - No byte beyond these is written: entries of d_pairs and d_pair_votes at or past the pairs written stay untouched.
 *   - The host step: the chain's calls take `pairs` as a host array, so the caller reads d_summary[0 .. 1] and the first
 *     8 * d_summary[1] bytes of d_pairs once, and hands that array to misift_match_pairs_batch_i8, the homography and
 *     fundamental calls, misift_link_tracks_batch and the rest.  That is the one small host read the selection needs;
 *     the call itself reads nothing back.
 *   - Deterministic: the selection is an exact radix select, the scores are integers, the pair list a prefix sum:
 *     byte-identical from run to run whatever the dispatch order.
 *   - NULL ctx, d_recs, d_q, d_counts or output pointer; d_q not 16-byte aligned; nframes < 0 or above
 *     MISIFT_SELECT_MAX_FRAMES (the vote matrix stays at 64 MB or less); top outside [1, MISIFT_SELECT_MAX_TOP]; k < 1;
 *     min_votes < 1; max_pairs < 0; min_score or max_ambiguity NaN; d_offsets NULL with a negative stride; an output
 *     that shares a byte with another output or with an input: MISIFT_EINVAL, before anything is enqueued.  The outputs
 *     are taken at their stated sizes (d_pairs: 2 * max_pairs ints), d_counts and d_offsets at nframes ints, d_recs and
 *     d_q at nframes * stride records in a padded layout; with d_offsets their extent is device data, and only their
 *     first byte is tested.  nframes == 0 writes only the summary.
 *   - The call runs on the context stream and returns before the GPU work is done; no host synchronisation and no host
 *     read of any count.  Ordering behind batches in flight (K > 1): as misift_match_batch.
 *   - Six launches and no memset, whatever the data (select and gather, votes, pick, count, scan, emit; the votes and emit
 *     launches fall away with fewer than two frames, emit with max_pairs == 0, all but the scan with no frame); no
 *     workgroup waits for another.  Temp memory, from the library's own allocator, is sized from nframes and top only:
 *     nframes * top' * 128 bytes of gathered descriptors (top' = top rounded up to 32), nframes^2 keep flags, 24 bytes
 *     per frame, each part rounded up to 16, plus 16. */
#define MISIFT_SELECT_MAX_TOP 256
#define MISIFT_SELECT_MAX_FRAMES 4096
int misift_select_pairs_batch(misift_ctx *ctx, const void *d_recs, const int8_t *d_q /* 16-byte aligned */, int nframes,
                              const int *d_counts, const int *d_offsets, int stride,
                              int top, float min_score, float max_ambiguity, int min_votes, int k, int max_pairs,
                              int *d_sel,         /* nframes x top ints */
                              int *d_sel_counts,  /* nframes ints */
                              int *d_votes,       /* nframes x nframes ints */
                              int *d_pairs,       /* 2 x max_pairs ints */
                              int *d_pair_votes,  /* max_pairs ints */
                              int *d_summary);    /* 8 ints */

/* Feature tracks of a pair-indexed batch (no reference counterpart): the accepted matches of every pair of
 * misift_match_pairs_batch / misift_match_pairs_batch_i8 joined ACROSS pairs into connected components, on the device.
 * A track is one scene point seen in several frames; it is usable (consistent) iff no two of its records lie in one
 * frame.  pairs, d_rows, d_row_counts and max_pts are what the pair matcher took and produced (d_out, d_out_counts):
 * pair i = (f1, f2), its row r is the record d_rows + (i * max_pts + r), d_row_counts[i] its row count or -1.  Both
 * frames of every pair belong to ONE record batch (the d_recs1 == d_recs2 windows and exhaustive sets), described by
 * nframes, d_counts and d_offsets (NULL: stride): record r of frame f has the global index
 * g(f, r) = (d_offsets ? d_offsets[f] : f * stride) + r, and frame f holds max(d_counts[f], 0) records.  The records
 * themselves are not an argument: nothing but the rows, the counts and the offsets is read.
 *   - Row r of pair i is an edge g(f1, r) -- g(f2, m) iff r < min(d_row_counts[i], max(d_counts[f1], 0), max_pts), its
 *     match field m satisfies 0 <= m < max(d_counts[f2], 0), score > min_score and ambiguity < max_ambiguity (the gate
 *     of matching.cu:1035, as in misift_find_homography_batch) and, when max_error is finite, match_error < max_error
 *     (what misift_improve_homography_batch writes into those rows).  With max_error = +inf match_error is not read at
 *     all (the matchers leave it untouched).  A comparison with a NaN field is false.  A pair with d_row_counts[i] < 0
 *     contributes nothing.  A self edge is a no-op; pairs (f, f) are allowed (they can only make inconsistent tracks).
 *   - d_track, d_track_len and d_track_frames are max_records ints each and mirror the record index space (as d_q of
 *     misift_quantize_batch does).  For every valid record g: d_track[g] = the smallest global index of g's component
 *     (a record with no accepted edge labels itself); d_track_len[g] = the records of the component if d_track[g] == g,
 *     else 0; d_track_frames[g] = the distinct frames among them if d_track[g] == g, else 0.  A track is consistent iff
 *     len == frames.  Slots that are no frame's valid record (padding of a strided layout, anything at or above the
 *     end, frames of count -1) are never written.
 *   - A frame whose records do not all lie in [0, max_records) takes no part: no labels, and every edge touching it is
 *     dropped.
 *   - d_summary (8 ints): [0] accepted edges (rows are counted: duplicates count twice, self edges once), [1] tracks
 *     with len >= 2, [2] records in those tracks, [3] how many of those tracks are inconsistent, [4] the longest track
 *     (1 when every record is a singleton, 0 without records), [5] frames dropped for lying outside max_records,
 *     [6] = [7] = 0.
 *   - Deterministic: all four outputs are functions of the edge set alone (labels are minima, everything else an
 *     integer sum), so they are byte-identical from run to run, whatever the dispatch order and whatever
 *     MISIFT_DETERMINISTIC says.
 *   - NULL ctx, npairs < 0, nframes < 0, a frame index outside [0, nframes), NULL d_rows, d_row_counts, d_counts or
 *     output pointer, max_pts < 1, max_records < 1, d_offsets NULL with a negative stride, min_score or max_ambiguity
 *     NaN, max_error NaN or <= 0: MISIFT_EINVAL, before anything is enqueued.  npairs == 0 is no error: every valid
 *     record becomes a singleton.  nframes == 0 writes only the summary.
 *   - The call runs on the context stream and returns before the GPU work is done; `pairs` is host memory the library
 *     copies; no host synchronisation and no host read of any count.  Ordering behind batches in flight (K > 1): as
 *     misift_match_batch.
 *   - One memset and five launches, whatever npairs and whatever the data (init, hook, label, distinct frames,
 *     summary).  Temp memory is 20 bytes per record of max_records plus 16 per pair, from the library's own allocator;
 *     nothing is sized by max_records x nframes or by anything read from the device. */
int misift_link_tracks_batch(misift_ctx *ctx, int npairs, const int *pairs /* host, npairs x 2 */,
                             const void *d_rows, const int *d_row_counts, int max_pts,
                             int nframes, const int *d_counts, const int *d_offsets, int stride,
                             int max_records,
                             float min_score, float max_ambiguity, float max_error,
                             int *d_track, int *d_track_len, int *d_track_frames,
                             int *d_summary /* 8 ints */);

/* Pair poses linked into one frame (no reference counterpart): the pose counterpart of misift_link_tracks_batch.
 * misift_recover_pose_batch gives every pair its own (R, t) with |t| = 1 and depths in that pair's private unit.  Two
 * pairs that share an image see a common point at ONE depth in the shared camera, in two units: the ratio of the two
 * depths is the ratio of the two baselines.  This call takes a robust ratio per link of two pairs, propagates the scales
 * from a seed pair, and composes the scaled poses along a walk into a camera per image, X_i = R_i . X_world + t_i.  In the
 * chain: find -> improve -> misift_match_epipolar_batch -> improve -> recover_pose -> link_poses.
 *   pairs, d_rows, d_row_counts and max_pts are those of misift_match_pairs_batch / misift_link_tracks_batch: pair p =
 *   (pairs[2p], pairs[2p+1]), two image indices in [0, nimages); its row r is the record p * max_pts + r, indexed by the
 *   set-1 record, and the row's `match` field is the set-2 record.  d_pose (npairs x 12), d_num_front (npairs) and d_xyz
 *   (4 floats per row, indexed like the rows) are what misift_recover_pose_batch wrote for those rows with frame i = pair
 *   i.  n(p) = min(max(d_row_counts[p], 0), max_pts) rows of pair p take part.
 *   A row is ACCEPTED under the edge rule of misift_link_tracks_batch: match >= 0, score > min_score, ambiguity <
 *   max_ambiguity and, when max_error is finite, match_error < max_error; with max_error = +inf match_error is not read.
 *   A comparison with a NaN is false.
 *   links[3l..3l+2] = (p, q, kind).  Kind 0, CHAIN: pairs[2p+1] == pairs[2q], p's set-2 image is q's set-1 image, and row
 *   r of p points at row r' = match[r] of q.  Kind 1, FAN: pairs[2p] == pairs[2q], the pairs have the same set-1 image,
 *   and r' = r.  Two pairs that share only their set-2 image would need an inverse map of the matches: out of scope.
 *   The arithmetic is that of misift_recover_pose_batch: fp32, every operation rounded, only + - * /, no contraction,
 *   every three-term sum taken left to right as written.
 *   1. Ratio per link.  Row r < n(p) of link l is a SAMPLE iff 0 <= r' < n(q), both rows are accepted, z1 > 0 && z2 > 0
 *      (components 2 and 3 of d_xyz) for both rows, and rho = zq / zp (one division) is finite and > 0, where zq = z1 of
 *      row r' and zp = z2 of row r (CHAIN: the depth in the shared camera, in p's unit) or z1 of row r (FAN).  rho
 *      estimates |T_p| / |T_q|.  c = the number of samples; d_link_common[l] = c; d_link_ratio[l] = the sample of rank
 *      (c - 1) >> 1 in ascending order (the lower median; equal samples are equal bits, so ties need no rule) if c >=
 *      min_common, otherwise 0.  The result is one of the samples: it depends on the sample set alone and is
 *      byte-identical from run to run.  r' comes from device memory and is range-checked before it addresses anything.
 *   2. Usable pairs and scales.  Pair p is USABLE iff d_num_front[p] > 0 and its twelve pose floats are finite.
 *      scale[.] = 0; scale[seed_pair] = 1 if that pair is usable.  The links are taken ONCE each, in the order given.  A
 *      link whose ratio is 0 or one of whose pairs is not usable is skipped.  Otherwise: scale[p] > 0 && scale[q] == 0:
 *      scale[q] = scale[p] / rho; scale[q] > 0 && scale[p] == 0: scale[p] = scale[q] * rho; anything else: nothing.  A
 *      result that is not finite and > 0 is left at 0.  The caller orders the links outwards from the seed: a link met
 *      before either of its pairs has a scale is LOST, it is not visited again.  A cycle's closing link does nothing.
 *   3. Cameras.  The root image gets the identity and t = 0, d_cam_pair[root_image] = -1.  Every other image starts
 *      unset: twelve zeros and d_cam_pair = -2.  `walk` is visited once, in order.  For walk entry p = (a, b) with s =
 *      scale[p] > 0, a != b and pose (R, t):  a set and b unset: R_b = R . R_a, t_b = (R . t_a) + s*t, d_cam_pair[b] = p;
 *      b set and a unset: R_a = R^T . R_b, t_a = R^T . (t_b - s*t), d_cam_pair[a] = p; otherwise nothing (both set: the
 *      first placement wins; a pair listed twice places nothing the second time).  Each entry of a product is
 *      (m0*n0 + m1*n1) + m2*n2 over the summed index.  There is no re-orthonormalisation: drift is the caller's to
 *      measure (DESIGN.md gives it for a chain of 64).  A NaN result is stored as 0x7fc00000.
 *   - Outputs: d_link_ratio, d_link_common (nlinks each), d_pair_scale (npairs), d_cam (nimages x 12: R row-major, then
 *     t), d_cam_pair (nimages), d_summary (8 ints): [0] links with c >= min_common, [1] pairs with scale > 0, [2] images
 *     with a camera (the root included), [3] the smallest c among the links of [0], 0 if there is none, [4..7] = 0.
 *     d_rows, d_pose, d_num_front and d_xyz are not written.
 *   - NULL ctx; npairs, nlinks or nwalk < 0; nimages < 1; root_image outside [0, nimages); min_common < 1; max_pts < 1;
 *     min_score or max_ambiguity NaN; max_error NaN or <= 0; NULL d_pair_scale, d_cam, d_cam_pair or d_summary; with
 *     nlinks > 0 a NULL links, d_link_ratio or d_link_common; with nwalk > 0 a NULL walk; with npairs > 0 a NULL pairs,
 *     d_rows, d_row_counts, d_pose, d_num_front or d_xyz, an image index outside [0, nimages) or seed_pair outside
 *     [0, npairs); a link whose p or q is outside [0, npairs), whose kind is neither 0 nor 1 or whose image indices do
 *     not agree with its kind; a walk entry outside [0, npairs): MISIFT_EINVAL, before anything is enqueued.  npairs ==
 *     0 (seed_pair is then not looked at) and nlinks == 0 are no errors: the root, and with a usable seed whatever the
 *     walk reaches through it, are placed.
 *   - The call runs on the context stream and returns before the GPU work is done; the three host lists are copied; no
 *     host synchronisation and no host read.  Ordering behind batches in flight (K > 1): as misift_match_batch.
 *   - Two launches whatever the data: one 256-thread workgroup per link (a radix select over the 32 bits of rho, 8 bits
 *     per pass) plus one that prepares step 2, then one wavefront for steps 2 and 3.  Temp memory is 12 bytes per link,
 *     12 per pair and 4 per walk entry, plus 16, from the library's own allocator. */
int misift_link_poses_batch(misift_ctx *ctx, int npairs, const int *pairs /* host, npairs x 2 */, int nimages,
                            const void *d_rows, const int *d_row_counts, int max_pts,
                            float min_score, float max_ambiguity, float max_error,
                            const float *d_pose /* npairs x 12 */, const int *d_num_front /* npairs */,
                            const float *d_xyz /* 4 floats per row */,
                            int nlinks, const int *links /* host, nlinks x 3: p, q, kind */,
                            int seed_pair, int root_image, int min_common,
                            int nwalk, const int *walk /* host, nwalk pair indices */,
                            float *d_link_ratio  /* nlinks */,
                            int   *d_link_common /* nlinks */,
                            float *d_pair_scale  /* npairs */,
                            float *d_cam         /* nimages x 12 */,
                            int   *d_cam_pair    /* nimages */,
                            int   *d_summary     /* 8 ints */);

/* The feature tracks of misift_link_tracks_batch as compact observation lists (no reference counterpart): the selected
 * tracks numbered in ascending order of their root, each with its observations (frame, record, xpos, ypos) stored
 * contiguously in ascending order of the global index, on the device.  It is the last call of the device-batch chain
 * extract -> quantize -> match -> find -> improve -> link -> export.
 *   - Frames, layouts (d_offsets, or stride when d_offsets is NULL), max(d_counts[f], 0) records per frame, the global
 *     index g(f, r), max_records and the rule "a frame whose records do not all lie in [0, max_records) takes no part"
 *     are exactly those of misift_link_tracks_batch.  d_track, d_track_len and d_track_frames are what that call wrote
 *     for the same layout and max_records.  Of d_recs only xpos and ypos are read, and only for records that are
 *     written out.
 *   - A valid record g is a root iff d_track[g] == g.  A root is selected iff d_track_len[g] >= min_len and, with
 *     consistent_only, d_track_len[g] == d_track_frames[g].  Selected tracks are numbered t = 0, 1, ... in ascending
 *     order of their root; off[t] = the sum of the lengths of the selected tracks before t.
 *   - Capacity: track t is written iff t < max_tracks and off[t] + len[t] <= max_obs.  off is increasing, so the
 *     written tracks are a prefix of T tracks holding O observations; no track is ever cut in the middle.
 *   - d_track_offsets[0 .. T] = off[0 .. T] (d_track_offsets[0] = 0 always); d_track_root[t] = the root, t < T;
 *     d_obs[off[t] + k], k < len[t] = the member of track t with the k-th smallest global index: its frame, its
 *     frame-local record index, and the bits of its xpos / ypos.  d_record_obs[g], when the pointer is given, is written
 *     for every valid record: that record's slot in d_obs, or -1 if its track is not written.  Every other byte of the
 *     four arrays stays untouched: entries at or beyond T + 1, T and O, slots that are no frame's valid record, frames
 *     that take no part.
 *   - d_summary (8 ints): [0] selected tracks, before the capacity rule, [1] their observations, [2] T, the tracks
 *     written, [3] O, the observations written, [4] the longest written track (0 if none), [5] frames dropped for lying
 *     outside max_records, [6] = [7] = 0.  [0] != [2] tells that something was cut.
 *   - Deterministic: every output is a function of the inputs alone (numbers and offsets are prefix sums of integers,
 *     a member's place is its rank by index), byte-identical from run to run whatever the dispatch order.
 *   - Every index that comes from device memory (counts, offsets, labels, lengths) is range-checked before it is used
 *     as an address.  Label arrays that no misift_link_tracks_batch call produced give unspecified contents, but never
 *     a write outside the capacities given nor a read outside [0, max_records) of the label arrays.
 *   - NULL ctx, nframes < 0, NULL d_recs, d_counts, label array, d_track_offsets, d_track_root, d_obs or d_summary,
 *     d_obs not 16-byte aligned, max_records < 1, min_len < 1, max_tracks < 1, max_obs < 1, consistent_only other than
 *     0 or 1, d_offsets NULL with a negative stride, d_record_obs equal to one of the three label arrays:
 *     MISIFT_EINVAL, before anything is enqueued.  nframes == 0 is no error: only d_summary and d_track_offsets[0] are
 *     written.
 *   - The call runs on the context stream and returns before the GPU work is done; no host synchronisation and no host
 *     read of any count.  Ordering behind batches in flight (K > 1): as misift_match_batch.
 *   - One memset and six launches, whatever the data (select, reduce per tile, scan of the tile sums, apply, place,
 *     write); no workgroup waits for another.  Temp memory is 16 bytes per record of max_records plus 8 per 2048
 *     records, from the library's own allocator; nothing is sized by anything read from the device. */
typedef struct misift_track_obs {   /* 16 bytes */
  int32_t frame;                    /* frame of the batch */
  int32_t record;                   /* frame-local record index r: global index g = base(frame) + r */
  float   xpos, ypos;               /* the record's xpos / ypos, bits copied */
} misift_track_obs;

int misift_export_tracks_batch(misift_ctx *ctx,
                               const void *d_recs, int nframes, const int *d_counts, const int *d_offsets, int stride,
                               int max_records,
                               const int *d_track, const int *d_track_len, const int *d_track_frames,
                               int min_len, int consistent_only,
                               int max_tracks, int max_obs,
                               int *d_track_offsets,        /* max_tracks + 1 ints */
                               int *d_track_root,           /* max_tracks ints */
                               misift_track_obs *d_obs,     /* max_obs entries, 16-byte aligned */
                               int *d_record_obs,           /* max_records ints, may be NULL */
                               int *d_summary);             /* 8 ints */

/* The exported tracks triangulated under the linked cameras (no reference counterpart): the call that joins the track
 * chain (... -> link_tracks -> export_tracks) to the pose chain (... -> recover_pose -> link_poses).  For every track
 * that misift_export_tracks_batch wrote, one world point from all of its views at once, refined on reprojection error,
 * and each observation's residual.  d_xyz of misift_recover_pose_batch is two-view, per pair and in the pair's own unit
 * and frame; d_points is N-view, in the frame and unit of d_cam.
 *   d_track_offsets, d_obs and d_export_summary are what misift_export_tracks_batch wrote for max_tracks and max_obs;
 *   obs.frame is the image index, so the batch's frames are the images of misift_link_poses_batch, whose d_cam
 *   (X_i = R_i . X_world + t_i, R row-major, then t) and d_cam_pair (-2 = the image has no camera) are read as written.
 *   intrinsics[4i..4i+3] = fx fy cx cy of image i.  obs.record is not read.
 *   The arithmetic is that of misift_recover_pose_batch: fp32, every operation rounded, only + - * / and sqrtf, no
 *   contraction, a comparison with a NaN is false.  Every sum over the observations runs in ascending k, starts at 0 and
 *   adds one term at a time; everything else is taken left to right as written.
 *   T = min(max(d_export_summary[2], 0), max_tracks), read on the device.  Entries at or beyond T of d_points,
 *   d_point_views and d_point_status, and entries of d_obs_error that belong to no track t < T, stay untouched.
 *   Track t < T has off = d_track_offsets[t] and end = d_track_offsets[t + 1], range-checked before they address
 *   anything: unless 0 <= off <= end <= max_obs the track gets status 4, four quiet NaNs and 0 views, and nothing of
 *   d_obs_error.  Otherwise its observations are o_k = d_obs[off + k], k < end - off.
 *   1. Usable views.  o_k is USABLE iff its frame f lies in [0, nimages), d_cam_pair[f] != -2, the twelve floats of
 *      d_cam[12f..] are finite, and x and y are finite.  m = the number of usable views; m < min_views: status 1.  Two
 *      observations from one frame (an inconsistent track) are both used.  Only usable views enter steps 2 - 4.
 *   2. Linear start.  With r0, r1, r2 the rows of R_f and (fx, fy, cx, cy) of image f: u = (x - cx) / fx, v =
 *      (y - cy) / fy; the first row is a = r0 - u*r2 (per component) with rhs = u*t2 - t0, the second a = r1 - v*r2 with
 *      rhs = v*t2 - t1.  Per row, in this order: M00 += a0*a0, M01 += a0*a1, M02 += a0*a2, M11 += a1*a1, M12 += a1*a2,
 *      M22 += a2*a2, g0 += a0*rhs, g1 += a1*rhs, g2 += a2*rhs; the u row before the v row.  SOLVE (M, g) -> X by LDL^T
 *      without pivoting: d0 = M00; l10 = M01/d0, l20 = M02/d0; d1 = M11 - l10*M01; e = M12 - l20*M01, l21 = e/d1;
 *      d2 = (M22 - l20*M02) - l21*e; y0 = g0, y1 = g1 - l10*y0, y2 = (g2 - l20*y0) - l21*y1; X2 = y2/d2,
 *      X1 = y1/d1 - l21*X2, X0 = (y0/d0 - l10*X1) - l20*X2.  The solve FAILS at the first pivot d0, d1, d2 that is not
 *      finite and > 0 (nothing is divided by it), or when a component of X is not finite.  A failed solve here: status 2.
 *   3. Residuals under X.  Per usable view: Xc.x = ((r00*X0 + r01*X1) + r02*X2) + t0, Xc.y and Xc.z likewise from r1, t1
 *      and r2, t2.  If Xc.z > 0 is false for a view, the point is NOT IN FRONT; after the linear start that is status 3.
 *      iz = 1/Xc.z, a = Xc.x*iz, b = Xc.y*iz; ru = x - (fx*a + cx), rv = y - (fy*b + cy); c += (ru*ru + rv*rv);
 *      Ju = (fx*iz) * (r0 - a*r2), Jv = (fy*iz) * (r1 - b*r2), per component; M and g take the row Ju with rhs ru, then
 *      the row Jv with rhs rv, as in step 2.
 *   4. Gauss-Newton, num_loops times at the most: SOLVE (M, g) -> delta; X' = X + delta per component; step 3 under X'
 *      gives c', M', g'.  X' is kept (with c', M', g') iff the solve did not fail, every usable view is in front under X'
 *      and c' < c; otherwise the loop ends there: "kept only if not worse", as misift_improve_fundamental_batch.
 *      num_loops = 0 gives the linear start.
 *   5. Outputs.  Status 0: d_points[4t..4t+3] = X0, X1, X2, sqrtf(c / (float)m), the rms reprojection error in pixels;
 *      d_point_views[t] = m; d_obs_error[off + k] = sqrtf(ru*ru + rv*rv) under the final X for a usable view, the quiet
 *      NaN 0x7fc00000 for any other.  Status 1, 2, 3: four quiet NaNs, d_point_views[t] = m, and the NaN for all of the
 *      track's d_obs_error.  d_point_status[t] = the status.  A single result that is a NaN is stored as 0x7fc00000.
 *      d_summary (8 ints, integer sums, so deterministic): [0] T, [1] tracks with status 0, [2] their usable views,
 *      [3] tracks with status 1, [4] with status 2, [5] with status 3, [6] Gauss-Newton steps kept, [7] tracks with
 *      status 4.
 *   - Not done here: no view is rejected as an outlier (misift_filter_tracks_batch does that on the device, then call
 *     this again), the cameras are not
 *     adjusted, and d_cam is used as it is, without re-orthonormalising its rotations: misift_refine_cameras_batch does
 *     both and hands back cameras for the next call of this one.
 *   - NULL ctx; max_tracks, max_obs or nimages < 1; NULL d_track_offsets, d_obs, d_export_summary, d_cam, d_cam_pair,
 *     intrinsics, d_points, d_point_views, d_point_status or d_summary; d_obs not 16-byte aligned; min_views < 2;
 *     num_loops < 0; an fx or fy that is not finite and > 0 or a cx or cy that is not finite: MISIFT_EINVAL, before
 *     anything is enqueued.  d_obs_error may be NULL.  None of the inputs is written.
 *   - The call runs on the context stream and returns before the GPU work is done; `intrinsics` is copied; no host
 *     synchronisation and no host read.  Ordering behind batches in flight (K > 1): as misift_match_batch.
 *   - One memset and one launch whatever the data: one lane per track, the grid sized from max_tracks.  The cameras and
 *     intrinsics are held on chip for up to 512 images; beyond that they are read from device memory, the intrinsics
 *     from a copy in 16 bytes per image of temp memory from the library's own allocator. */
int misift_triangulate_tracks_batch(misift_ctx *ctx,
                                    int max_tracks, int max_obs,
                                    const int *d_track_offsets,     /* max_tracks + 1, from export */
                                    const misift_track_obs *d_obs,  /* max_obs, from export, 16-byte aligned */
                                    const int *d_export_summary,    /* 8 ints, from export: [2] = T */
                                    int nimages,
                                    const float *d_cam,             /* nimages x 12, from link_poses */
                                    const int *d_cam_pair,          /* nimages, from link_poses */
                                    const float *intrinsics,        /* host, nimages x 4: fx fy cx cy, copied */
                                    int min_views, int num_loops,
                                    float *d_points,                /* max_tracks x 4: X Y Z, rms error in px */
                                    int   *d_point_views,           /* max_tracks */
                                    int   *d_point_status,          /* max_tracks */
                                    float *d_obs_error,             /* max_obs, may be NULL */
                                    int   *d_summary);              /* 8 ints */

/* The linked cameras refined against the triangulated track points (no reference counterpart): the other half of the
 * minimisation of misift_triangulate_tracks_batch.  With the points held, each camera is moved to minimise the
 * reprojection error of the observations its image makes (motion-only bundle adjustment, resection refinement).
 * Alternated with misift_triangulate_tracks_batch this is block-coordinate bundle adjustment, all of it on the device.
 *   d_track_offsets, d_obs and d_export_summary are what misift_export_tracks_batch wrote for max_tracks and max_obs,
 *   d_points and d_point_status what misift_triangulate_tracks_batch wrote for them, d_cam and d_cam_pair what
 *   misift_link_poses_batch (or an earlier call of this one) wrote; intrinsics[4i..4i+3] = fx fy cx cy of image i.
 *   `hold` lists nhold image indices whose cameras are kept as they are (an index may repeat).  Held cameras fix the
 *   gauge: the root is always kept, and the caller normally holds the other image of the seed pair as well, so that the
 *   scale cannot creep when this call and triangulate alternate.  obs.record and d_points[4t+3] are not read.
 *   The arithmetic is that of misift_triangulate_tracks_batch: fp32, every operation rounded, only + - * / and sqrtf, no
 *   contraction, a comparison with a NaN is false, everything taken left to right as written; a . b of two 3-vectors is
 *   (a0*b0 + a1*b1) + a2*b2.  A single result that is a NaN is stored as 0x7fc00000.
 *   Owner of a slot.  T = min(max(d_export_summary[2], 0), max_tracks) and O = min(max(d_export_summary[3], 0), max_obs),
 *   both read on the device.  Track t < T is VALID iff 0 <= off[t] <= off[t + 1] <= O, checked before it addresses
 *   anything.  The OWNER of slot o < O is the largest valid t with off[t] <= o < off[t + 1], or none.  Under export's own
 *   output the ranges are disjoint; the rule only makes hostile offsets deterministic.
 *   Candidates.  Slot o < O is a CANDIDATE of image i iff it has an owner t, d_obs[o].frame == i, d_point_status[t] == 0,
 *   X = d_points[4t..4t+2] is finite, and d_obs[o].xpos and .ypos (x, y below) are finite.
 *   The sum of the call is the rule of misift_improve_fundamental_batch with the slot index o in place of the record
 *   index: p[s], s < 256, starts at +0 and adds the terms of the members with o = s (mod 256) in ascending o, one at a
 *   time (a slot that is no member is skipped); then for off = 128, 64 ... 1: p[s] = p[s] + p[s + off] for s < off; the
 *   sum is p[0].
 *   Per image i, independently of every other image:
 *   0. Status without work.  d_cam_pair[i] == -2, or one of the twelve floats d_cam[12i..] not finite: status 4.
 *      Otherwise d_cam_pair[i] == -1 (the root) or i in `hold`: status 3.  Either way d_cam_out[12i..] gets the twelve
 *      floats bit for bit, d_cam_obs[i] = 0, d_cam_steps[i] = 0 and both d_cam_rms entries the quiet NaN.
 *   1. Orthonormalise, when orthonormalise == 1.  With r0, r1, r2 the rows of R: n0 = sqrtf(r0 . r0), r0 <- r0 / n0 per
 *      component; d = r1 . r0 (the new r0), w = r1 - d*r0 per component, n1 = sqrtf(w . w), r1 <- w / n1; r2 <- r0 x r1
 *      with components r0[1]*r1[2] - r0[2]*r1[1], r0[2]*r1[0] - r0[0]*r1[2], r0[0]*r1[1] - r0[1]*r1[0].  t is unchanged.
 *      A non-finite result: status 4, with the outputs of step 0.  With orthonormalise == 0 the camera is as given.
 *   2. Members, under the camera (R, t) of step 1.  Per candidate, as step 3 of misift_triangulate_tracks_batch:
 *      Xc.x = ((r00*X0 + r01*X1) + r02*X2) + t0, Xc.y and Xc.z likewise; iz = 1/Xc.z, a = Xc.x*iz, b = Xc.y*iz;
 *      ru = x - (fx*a + cx), rv = y - (fy*b + cy).  The candidate is a MEMBER iff Xc.z > 0 and ru*ru + rv*rv < E2, where
 *      E2 = max_error*max_error is rounded once on the host; when E2 is +inf the test is Xc.z > 0 alone.  The member set
 *      is fixed here and does not change in the loops.  n = its size.  n < min_obs: status 1; the camera of step 1 is
 *      written, d_cam_obs[i] = n, both d_cam_rms entries are the quiet NaN and d_cam_steps[i] = 0.
 *   3. Cost and normal equations under a camera (R, t), over the members.  Xc, iz, a, b, ru, rv as in step 2 under
 *      (R, t); gx = fx*iz, gy = fy*iz; the parameters are (wx wy wz ux uy uz), a rotation and a translation of the
 *      camera frame:
 *        Ju = ( gx*(-(a*Xc.y)), gx*(Xc.z + a*Xc.x), gx*(-Xc.y), gx*1, gx*0, gx*(-a) )
 *        Jv = ( gy*(-(Xc.z + b*Xc.y)), gy*(b*Xc.x), gy*Xc.x, gy*0, gy*1, gy*(-b) )
 *      28 sums of the call: c with the term ru*ru + rv*rv; M[r][q] for r <= q < 6 with the term Ju[r]*Ju[q] + Jv[r]*Jv[q]
 *      (M[q][r] = M[r][q]); g[r] with the term Ju[r]*ru + Jv[r]*rv.  A member with Xc.z > 0 false makes the camera NOT IN
 *      FRONT; its sums are not used.
 *   4. SOLVE M delta = g by LDL^T without pivoting.  For j = 0 ... 5 in turn: v_k = L[j][k]*d_k for k < j;
 *      d_j = M[j][j] - L[j][0]*v_0 - ... - L[j][j-1]*v_(j-1), one subtraction at a time in ascending k; then for every
 *      i > j: L[i][j] = (M[i][j] - L[i][0]*v_0 - ... - L[i][j-1]*v_(j-1)) / d_j, the same way.  y_i = g[i] - L[i][0]*y_0
 *      - ... - L[i][i-1]*y_(i-1) for i = 0 ... 5; delta_i = y_i/d_i - L[i+1][i]*delta_(i+1) - ... - L[5][i]*delta_5 for
 *      i = 5 ... 0, the quotient first, then ascending k.  The solve FAILS at the first pivot d_j that is not finite and
 *      > 0 (nothing is divided by it), or when a component of delta is not finite.
 *   5. Update by the Cayley map, which is rational and, in exact arithmetic, orthogonal.  h = 0.5*(wx, wy, wz) per
 *      component, s = h . h, e = 1 - s, q = 1 + s;
 *        C00 = (e + 2*(h0*h0))/q        C01 = (2*(h0*h1) - 2*h2)/q     C02 = (2*(h0*h2) + 2*h1)/q
 *        C10 = (2*(h0*h1) + 2*h2)/q     C11 = (e + 2*(h1*h1))/q        C12 = (2*(h1*h2) - 2*h0)/q
 *        C20 = (2*(h0*h2) - 2*h1)/q     C21 = (2*(h1*h2) + 2*h0)/q     C22 = (e + 2*(h2*h2))/q
 *      R'[r][c] = (C[r][0]*R[0][c] + C[r][1]*R[1][c]) + C[r][2]*R[2][c];
 *      t'[r] = ((C[r][0]*t0 + C[r][1]*t1) + C[r][2]*t2) + u_r.
 *   6. Gauss-Newton.  Step 3 under the camera of step 1 gives c0 = c, M, g.  Then num_loops times at the most: SOLVE,
 *      update, step 3 under (R', t') gives c', M', g'.  (R', t') is kept (with c', M', g') iff the solve did not fail,
 *      the camera is in front of every member and c' < c; otherwise the loop ends there.  Status 2 iff the first solve
 *      fails; the camera of step 1 is written.  Otherwise status 0.  num_loops = 0 solves nothing.
 *   7. Outputs.  d_cam_out[12i..12i+11] = the last camera kept (the twelve input floats bit for bit when nothing was
 *      kept and orthonormalise == 0); d_cam_obs[i] = n; d_cam_rms[2i] = sqrtf(c0 / (float)n) and d_cam_rms[2i + 1] =
 *      sqrtf(c / (float)n) under the camera written, in pixels; d_cam_steps[i] = the steps kept; d_cam_status[i].
 *      d_summary (8 ints, integer sums, so deterministic): [0] T, [1] cameras with status 0, [2] their members,
 *      [3] cameras with status 1, [4] with status 2, [5] with status 3, [6] steps kept, [7] cameras with status 4.
 *   - With num_loops == 0 and orthonormalise == 0 every camera comes back bit for bit, and d_cam_rms[2i] is the
 *     per-image rms that d_obs_error of misift_triangulate_tracks_batch implies (over the members, under max_error).
 *   - Not done here: camera and point steps are not taken jointly (no Schur complement: misift_adjust_bundle_batch does
 *     that; or alternate with triangulate), no robust kernel re-weights a residual (max_error is a hard gate, decided once;
 *     misift_filter_tracks_batch revises the lists between calls), and the intrinsics are
 *     not refined (misift_adjust_bundle_focal_batch refines a focal scale per camera).
 *   - NULL ctx; max_tracks, max_obs or nimages < 1; NULL d_track_offsets, d_obs, d_export_summary, d_points,
 *     d_point_status, d_cam, d_cam_pair, intrinsics, d_cam_out, d_cam_obs, d_cam_rms, d_cam_steps, d_cam_status or
 *     d_summary; d_obs not 16-byte aligned; min_obs < 3; num_loops < 0; max_error NaN or <= 0; orthonormalise other than
 *     0 or 1; nhold < 0, nhold > 0 with NULL hold, a hold index outside [0, nimages); an fx or fy that is not finite and
 *     > 0 or a cx or cy that is not finite; d_cam_out overlapping d_cam without being equal to it: MISIFT_EINVAL, before
 *     anything is enqueued.  hold may be NULL when nhold == 0.  None of the inputs is written, except d_cam when it is
 *     d_cam_out.
 *   - The call runs on the context stream and returns before the GPU work is done; `intrinsics` and `hold` are copied;
 *     no host synchronisation and no host read.  Ordering behind batches in flight (K > 1): as misift_match_batch.
 *   - Two memsets and three launches whatever the data: one lane per track finds the owners, one lane per slot the
 *     candidates, then one 256-thread workgroup per image, its thread s being slot s of the sum.  8 bytes per slot of
 *     temp memory from the library's own allocator, sized from max_obs only. */
int misift_refine_cameras_batch(misift_ctx *ctx,
                                int max_tracks, int max_obs,
                                const int *d_track_offsets,     /* max_tracks + 1, from export */
                                const misift_track_obs *d_obs,  /* max_obs, from export, 16-byte aligned */
                                const int *d_export_summary,    /* 8 ints, from export: [2] = T, [3] = O */
                                const float *d_points,          /* max_tracks x 4, from triangulate */
                                const int *d_point_status,      /* max_tracks, from triangulate */
                                int nimages,
                                const float *d_cam,             /* nimages x 12, from link_poses */
                                const int *d_cam_pair,          /* nimages, from link_poses */
                                const float *intrinsics,        /* host, nimages x 4: fx fy cx cy, copied */
                                int nhold, const int *hold,     /* host, images kept as they are, copied; may be NULL */
                                int min_obs, int num_loops, float max_error, int orthonormalise,
                                float *d_cam_out,               /* nimages x 12; may be d_cam itself */
                                int   *d_cam_obs,               /* nimages */
                                float *d_cam_rms,               /* nimages x 2: before, after */
                                int   *d_cam_steps,             /* nimages */
                                int   *d_cam_status,            /* nimages */
                                int   *d_summary);              /* 8 ints */

/* The camera of an image estimated directly from the observations it makes of the triangulated track points, robustly
 * (resection; no reference counterpart).  misift_link_poses_batch is the only other origin of a camera: an image its walk
 * does not reach stays at d_cam_pair == -2 although its observations of known points sit in d_obs, and a camera it does
 * place rests on one chain of two-view estimates, which misift_refine_cameras_batch can polish but not replace.  This call
 * runs, per selected image, a RANSAC search over calibrated six-point solves and counts inliers with the member test of
 * misift_refine_cameras_batch.  In the chain: ... export -> triangulate -> resect -> triangulate -> refine <-> triangulate.
 *   d_track_offsets, d_obs and d_export_summary are what misift_export_tracks_batch wrote for max_tracks and max_obs,
 *   d_points and d_point_status what misift_triangulate_tracks_batch wrote for them; intrinsics[4i..4i+3] = fx fy cx cy
 *   of image i.  Entry e < nsel works on image i = images[e] with the seed seeds[e] and writes result slot e.
 *   obs.record and d_points[4t+3] are not read.
 *   The arithmetic is that of misift_refine_cameras_batch: fp32, every operation rounded, only + - * /, sqrtf and fabsf,
 *   no contraction, a comparison with a NaN is false, everything taken left to right as written.  A single result that
 *   is a NaN is stored as 0x7fc00000.  FINITE means fabsf(v) <= FLT_MAX.
 *   T, O, valid tracks, the OWNER of a slot and the CANDIDATES of an image are those of misift_refine_cameras_batch,
 *   word for word.
 *   Per entry e, independently of every other entry:
 *   1. Skip.  only_unset == 1 and d_cam_pair[i] != -2 (read on the device): status 3; d_res_cam[12e..] gets twelve zeros,
 *      d_res_cand[e] = 0, d_res_inliers[e] = 0, and nothing else is done.
 *   2. Candidates.  The candidates of image i in ascending slot index o; candidate p < n has (x, y) = d_obs[o_p].xpos,
 *      .ypos and (X, Y, Z) = d_points[4t..4t+2] of the owner t of o_p.  d_res_cand[e] = n.  n > max_cand: status 4;
 *      n < max(6, min_inliers): status 1.  Either way twelve zeros and d_res_inliers[e] = 0.
 *   3. Draw.  rand() is glibc's after srand(seeds[e]) (as misift_find_homography_batch restates it).  The num_loops
 *      hypotheses are drawn one after another from the one stream.  A hypothesis is six positions p_0 .. p_5: first
 *      p_k = rand() % n for k = 0 .. 5; then for k = 1 .. 5 in turn, while p_k equals one of p_0 .. p_(k-1):
 *      p_k = rand() % n.
 *   4. Solve, per hypothesis, with (x_k, y_k, X_k, Y_k, Z_k) the candidate at position p_k:
 *      a. u_k = (x_k - cx) / fx, v_k = (y_k - cy) / fy.  World normalisation: SX = 0 + X_0 + ... + X_5 one at a time,
 *         SY and SZ likewise; c = (SX / 6, SY / 6, SZ / 6); dX = X_k - c0, dY = Y_k - c1, dZ = Z_k - c2;
 *         d = 0 + sqrtf((dX*dX + dY*dY) + dZ*dZ) over k = 0 .. 5 one at a time; s = 10.3923048f / d (6 sqrt(3): the mean
 *         distance to c becomes sqrt(3)); a_k = dX * s, b_k = dY * s, w_k = dZ * s.
 *      b. The 11 x 12 system in the entries of P = [M | p], row-major 3 x 4 (column 4r + q holds P[r][q]).  Row 2k, the
 *         u-row of point k = 0 .. 5:  ( a_k  b_k  w_k  1   0 0 0 0   -(u_k*a_k)  -(u_k*b_k)  -(u_k*w_k)  -u_k );
 *         row 2k + 1, the v-row of point k = 0 .. 4:  ( 0 0 0 0   a_k  b_k  w_k  1   -(v_k*a_k)  -(v_k*b_k)  -(v_k*w_k)
 *         -v_k ).  Point 5 has no v-row.  The null vector by the rule of step 2 of misift_find_fundamental_batch at
 *         11 x 12: Gaussian elimination with complete pivoting, eleven steps; at step j the pivot is the entry of rows
 *         j..10 x columns j..11 with the largest fabsf, searched row-major with a strict '>' (the first maximum wins, a
 *         NaN never does; when nothing wins, the entry (j, j)); rows j and the pivot's change places, then the columns;
 *         for every row r > j: f = A[r][j] / A[j][j], A[r][q] = A[r][q] - f * A[j][q] for q > j.  Then z_11 = 1 and, for
 *         j = 10 .. 0, z_j = (-(0 + A[j][j+1]*z_(j+1) + ... + A[j][11]*z_11)) / A[j][j], the sum one term at a time in
 *         ascending q; P = z with the column permutation undone.  A pivot that is zero or not FINITE makes the
 *         hypothesis INVALID.
 *      c. m = the largest fabsf of the twelve entries of P; an entry that is not FINITE, or m == 0: INVALID.
 *         P = P / m per entry.  det = (P00*(P11*P22 - P12*P21) - P01*(P10*P22 - P12*P20)) + P02*(P10*P21 - P11*P20);
 *         det == 0 or not FINITE: INVALID; det < 0: every entry of P is negated.
 *         A = M (the left 3 x 3 of P), V = I; six sweeps of the one-sided Jacobi rotation of step 2 of
 *         misift_recover_pose_batch over the column pairs (0,1), (0,2), (1,2), applied to A and V alike.
 *         sigma_j = sqrtf(A0j*A0j + A1j*A1j + A2j*A2j); a sigma_j that is not FINITE and > 0: INVALID.
 *         U[r][j] = A[r][j] / sigma_j; R[r][q] = (U[r][0]*V[q][0] + U[r][1]*V[q][1]) + U[r][2]*V[q][2], the nearest
 *         rotation to M.  lambda = ((sigma_0 + sigma_1) + sigma_2) / 3; tn_r = P[r][3] / lambda;
 *         t_r = tn_r / s - ((R[r][0]*c0 + R[r][1]*c1) + R[r][2]*c2), which undoes the world normalisation.
 *         A component of (R, t) that is not FINITE: INVALID.
 *      An INVALID hypothesis is twelve zeros, which no candidate fits (step 5 needs Xc.z > 0).
 *   5. Count.  A candidate is an INLIER of a hypothesis (R, t) iff it is a MEMBER under it by step 2 of
 *      misift_refine_cameras_batch with E2 = thresh*thresh rounded once on the host: Xc.z > 0 and ru*ru + rv*rv < E2
 *      (E2 = +inf: Xc.z > 0 alone).  The count of a hypothesis runs over all n candidates.
 *   6. Pick.  The hypothesis with the largest count, the smallest index among equals.  d_res_inliers[e] = its count.
 *      count < min_inliers: status 2 and twelve zeros.  Otherwise status 0 and d_res_cam[12e..12e+11] = its R row-major,
 *      then t (X_i = R . X_world + t, as d_cam).
 *   7. Install.  install == 1 and status 0: d_cam[12i..12i+11] = the twelve floats and d_cam_pair[i] = -3,
 *      MISIFT_CAM_RESECTED ("placed by resection").  misift_triangulate_tracks_batch and misift_refine_cameras_batch
 *      treat every value but -2 as "has a camera" and only -1 as the root.  With any other status, or install == 0,
 *      d_cam and d_cam_pair are not written.
 *   d_res_status[e] = the status.  d_summary (8 ints, integer sums, so deterministic): [0] T, [1] entries with status 0,
 *   [2] their inliers, [3] entries with status 1, [4] with status 2, [5] with status 3, [6] with status 4, [7] 0.
 *   - Not done here: no minimal (P3P) solver: the six-point solve is degenerate for coplanar points, so a scene whose
 *     points lie in a plane ends in status 2, and an image that sees the scene mostly through a plane may do so too.  No
 *     local optimisation inside the search: misift_refine_cameras_batch with max_error = thresh is the polish.  The
 *     intrinsics are taken as given.
 *   - NULL ctx; max_tracks, max_obs or nimages < 1; NULL d_track_offsets, d_obs, d_export_summary, d_points,
 *     d_point_status, intrinsics, d_res_cam, d_res_cand, d_res_inliers, d_res_status or d_summary; NULL d_cam_pair with
 *     only_unset or install set, NULL d_cam with install set; d_obs not 16-byte aligned; nsel < 0, nsel > 0 with NULL
 *     images or seeds, an image index outside [0, nimages) or listed twice; max_cand < 6; num_loops < 1; thresh NaN or
 *     <= 0; min_inliers < 6; only_unset or install other than 0 or 1; an fx or fy that is not finite and > 0 or a cx or
 *     cy that is not finite; nsel x ceil(num_loops / 64) x ceil(min(max_cand, max_obs) / 512) beyond 2^31 - 1 (one
 *     launch), or num_loops beyond 2^31 - 16: MISIFT_EINVAL, before anything is enqueued.  nsel == 0 is no error: only
 *     d_summary is written.  None of the inputs is written, except d_cam and d_cam_pair under install.
 *   - The call runs on the context stream and returns before the GPU work is done; `intrinsics`, `images` and `seeds`
 *     are copied; no host synchronisation and no host read.  Ordering behind batches in flight (K > 1): as
 *     misift_match_batch.
 *   - Two memsets and six launches whatever the data: the owners and the candidates as misift_refine_cameras_batch finds
 *     them, then per entry the ordered candidate list and the draw, one lane per (entry, hypothesis) for the solve, one
 *     64-lane workgroup per (entry, 64 hypotheses, 512 candidates) for the count, and the pick.  Temp memory from the
 *     library's own allocator, sized from max_obs, nsel, max_cand and num_loops only: 8 bytes per slot, and per entry
 *     20 bytes per candidate of min(max_cand, max_obs) and 76 bytes per hypothesis (both rounded up to 16). */
#define MISIFT_CAM_RESECTED (-3)
int misift_resect_cameras_batch(misift_ctx *ctx,
                                int max_tracks, int max_obs,
                                const int *d_track_offsets,     /* max_tracks + 1, from export */
                                const misift_track_obs *d_obs,  /* max_obs, from export, 16-byte aligned */
                                const int *d_export_summary,    /* 8 ints, from export: [2] = T, [3] = O */
                                const float *d_points,          /* max_tracks x 4, from triangulate */
                                const int *d_point_status,      /* max_tracks, from triangulate */
                                int nimages,
                                const float *intrinsics,        /* host, nimages x 4: fx fy cx cy, copied */
                                int nsel, const int *images,    /* host, nsel distinct image indices, copied */
                                const unsigned *seeds,          /* host, nsel, copied */
                                int max_cand, int num_loops, float thresh /* px */, int min_inliers,
                                int only_unset, int install,
                                float *d_cam,                   /* nimages x 12: written when install */
                                int   *d_cam_pair,              /* nimages: read when only_unset, written when install */
                                float *d_res_cam,               /* nsel x 12 */
                                int   *d_res_cand,              /* nsel */
                                int   *d_res_inliers,           /* nsel */
                                int   *d_res_status,            /* nsel */
                                int   *d_summary);              /* 8 ints */

/* Two reconstructions related (no reference counterpart).  Everything the chain produces lives in one arbitrary gauge:
 * the frame of root_image and the unit of seed_pair.  The three calls below relate two such gauges: the other side of a
 * break in the walk of misift_link_poses_batch reconstructed from its own seed, overlapping windows of a long sequence,
 * a reconstruction against surveyed points.  misift_correspond_tracks_batch finds which points correspond,
 * misift_align_points_batch estimates the similarity transform b = s R a + t between them robustly, and
 * misift_transform_scene_batch applies it to points and cameras.
 * misift_merge_scenes_batch then writes the two scenes out as one, which every call of the track chain takes.
 *   - Not done here: no reprojection-error inlier test (the test is the 3-D distance in the units of d_dst); no
 *     camera-centre correspondences; no re-adjustment afterwards, which misift_adjust_bundle_* does on the merged scene.
 *
 * misift_correspond_tracks_batch: two exported scenes A and B over the same records (two link / export runs over different
 * pair sets of one record batch, or over two views into one packed batch).  Record g of A (its global index, as
 * d_record_obs of misift_export_tracks_batch is indexed) is record g - shift of B; shift == 0 means one batch.
 *   PRECONDITION: each d_record_obs was filled with -1 by the caller before its export, since export leaves the entries
 *   of invalid records untouched.  A stale entry can at worst make a wrong tie; it cannot make the call read or write out
 *   of bounds.
 *   T_A = min(max(d_export_summary_a[2], 0), max_tracks_a), O_A = min(max(d_export_summary_a[3], 0), max_obs_a), T_B and
 *   O_B likewise, all read on the device.
 *   The TRACK OF a slot o among T tracks with offsets off: T < 1: none.  Otherwise lo = 0, hi = T; while hi - lo > 1:
 *   mid = lo + (hi - lo) / 2, and off[mid] <= o ? lo = mid : hi = mid.  The track is lo iff off[lo] <= o < off[lo + 1],
 *   otherwise none (so hostile offsets only drop the record; only off[0 .. T] is read).
 *   Record g in [0, max_records_a) makes a TIE (t_A, t_B) iff 0 <= g - shift < max_records_b (in 64 bits),
 *   o_A = d_record_obs_a[g] lies in [0, O_A), o_B = d_record_obs_b[g - shift] lies in [0, O_B), t_A is the track of o_A
 *   among A's and t_B the track of o_B among B's, and both exist.
 *   d_map[t], t < T_A: -1 when no tie names t as t_A; the one t_B when all its ties name the same; -2 when they name
 *   several.  d_map at or beyond T_A stays untouched.  d_summary (8 ints): [0] T_A, [1] T_B, [2] ties, [3] tracks with
 *   d_map >= 0, [4] tracks with d_map == -2, [5..7] 0.
 *   - NULL ctx or pointer; a capacity < 1: MISIFT_EINVAL, before anything is enqueued.  None of the inputs is written.
 *   - Stream semantics as misift_resect_cameras_batch; no host read.  Three memsets and two launches whatever the data:
 *     one thread per record (atomicMin and atomicMax of t_B per t_A, which no order of the threads changes), one per
 *     track.  Temp memory from the library's own allocator: 8 bytes per track of max_tracks_a. */
int misift_correspond_tracks_batch(misift_ctx *ctx, int shift,
                                   int max_records_a, const int *d_record_obs_a,   /* max_records_a, from export A */
                                   int max_tracks_a, int max_obs_a,
                                   const int *d_track_offsets_a,                   /* max_tracks_a + 1 */
                                   const int *d_export_summary_a,                  /* 8 ints */
                                   int max_records_b, const int *d_record_obs_b,
                                   int max_tracks_b, int max_obs_b,
                                   const int *d_track_offsets_b, const int *d_export_summary_b,
                                   int *d_map,                                     /* max_tracks_a */
                                   int *d_summary);                                /* 8 ints */

/* misift_align_points_batch: per entry, the similarity transform (s, R, t) with b = s R a + t between corresponding 3-D
 * points, by RANSAC over three-point closed-form solves (Horn 1987 / Umeyama 1991), refitted over its inliers.
 *   d_src and d_dst are pooled arrays of four floats per point, X Y Z and a word that is not read (the format of
 *   d_points); d_src_status and d_dst_status, where given, hold 0 for a usable point (as d_point_status); d_map holds one
 *   int per source point.  Entry e < nsel has ranges[4e .. 4e+3] = src_first, src_cap, dst_first, dst_cap: its source
 *   points are d_src[4 (src_first + i)], i < src_cap, with d_map[src_first + i] beside them, and the correspondent of
 *   source point i is point dst_first + d_map[src_first + i] of d_dst.  n_e = src_cap when d_count is NULL, otherwise
 *   min(max(d_count[e * count_stride], 0), src_cap), read on the device (the export summaries of the entries laid end to
 *   end: d_count = summaries + 2, count_stride = 8 gives T).
 *   The arithmetic is that of misift_refine_cameras_batch: fp32, every operation rounded, only + - * /, sqrtf and fabsf,
 *   no contraction, a comparison with a NaN is false, everything taken left to right as written.  A single result that
 *   is a NaN is stored as 0x7fc00000.  FINITE means fabsf(v) <= FLT_MAX.
 *   Per entry e, independently of every other entry:
 *   1. Candidates.  Source point i < n_e is a CANDIDATE iff m = d_map[src_first + i] lies in [0, dst_cap),
 *      d_src_status[src_first + i] == 0 and d_dst_status[dst_first + m] == 0 where the arrays are given, and all six
 *      coordinates a = d_src[4 (src_first + i) .. + 2], b = d_dst[4 (dst_first + m) .. + 2] are FINITE.  The candidates in
 *      ascending i form the ordered list; candidate p < n.  d_align_cand[e] = n.  n < max(3, min_inliers): status 1,
 *      sixteen zeros, d_align_inliers[e] = 0.
 *   2. Draw.  rand() is glibc's after srand(seeds[e]) (as misift_find_homography_batch restates it).  The num_loops
 *      hypotheses are drawn one after another from the one stream.  A hypothesis is three positions: first
 *      p_k = rand() % n for k = 0, 1, 2; then for k = 1, 2 in turn, while p_k equals an earlier one: p_k = rand() % n.
 *   3. Solve (a_k, b_k the candidate at position p_k; K = 3 and the sums run over k = 0, 1, 2 one at a time from +0):
 *      a. Centroids: ca_j = (((0 + a_0j) + a_1j) + a_2j) / 3, cb likewise.  da_k = a_k - ca, db_k = b_k - cb.
 *      b. Per correspondence the eleven TERMS M[r][c] = db[r] * da[c] (r, c < 3), qa = (da0*da0 + da1*da1) + da2*da2 and
 *         qb likewise from db.  M, sa and sb are their sums.
 *      c. m = the largest fabsf of the nine entries of M; an entry that is not FINITE, or m == 0: INVALID.  A = M / m per
 *         entry, V = I; six sweeps of the one-sided Jacobi rotation of step 2 of misift_recover_pose_batch over the
 *         column pairs (0,1), (0,2), (1,2), applied to A and V alike.  w_j = A0j*A0j + A1j*A1j + A2j*A2j.  i1 = the
 *         column of the largest w, i2 that of the second largest, chosen as step 3 of misift_recover_pose_batch chooses
 *         them (strict '>', the first maximum wins; of the other two the later only if strictly larger).  w_i2 > 0 false, or
 *         w_i2 > w_i1 * 1e-10f false: INVALID (collinear or coincident points; the second gate, sigma2 / sigma1 <= 1e-5
 *         or about 84 eps, catches the sets that are collinear up to the roundings of M / m, whose second column is
 *         noise and need not even be orthogonal to the first.  The singular values of M go with the squares of the
 *         spreads: the gate turns away a point set more than about 300 times as long as it is wide, whose rotation
 *         about its long axis float32 would get wrong by a hundredth or more).
 *      d. u1 = column i1 of A / sqrtf(w_i1), u2 = column i2 of A / sqrtf(w_i2), v1, v2 = those columns of V;
 *         u3 = u1 x u2, v3 = v1 x v2 (x: (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0));
 *         R[r][c] = (u1[r]*v1[c] + u2[r]*v2[c]) + u3[r]*v3[c].  This is Umeyama's answer, the reflection case included: a
 *         proper rotation by construction, and well defined for three points, whose M has rank 2.
 *      e. sa == 0: INVALID.  s = sqrtf(sb / sa); s == 0 or not FINITE: INVALID.
 *         t_r = cb_r - s * ((R[r][0]*ca_0 + R[r][1]*ca_1) + R[r][2]*ca_2).  One of the thirteen numbers not FINITE:
 *         INVALID.
 *      An INVALID hypothesis is thirteen 0x7fc00000, which no candidate fits (zeros would fit points near the origin).
 *   4. Count.  E2 of a candidate under (R, t, s): p_r = s * ((R[r][0]*a_0 + R[r][1]*a_1) + R[r][2]*a_2) + t_r,
 *      d_r = b_r - p_r, E2 = (d_0*d_0 + d_1*d_1) + d_2*d_2.  It is a MEMBER iff E2 < thresh2, thresh2 = thresh * thresh
 *      rounded once on the host (thresh = +inf: every candidate with a FINITE E2).  The count of a hypothesis runs over
 *      all n candidates.
 *   5. Pick.  The hypothesis with the largest count, the smallest index among equals.  count < min_inliers: status 2,
 *      sixteen zeros, d_align_inliers[e] = that count.
 *   6. Refit, otherwise.  h = the picked transform, c = its count.  Up to refit_loops times: the members under h;
 *      S = the sum over them of (a_0 a_1 a_2 b_0 b_1 b_2); ca = S[0..2] / (float)c, cb = S[3..5] / (float)c, each one
 *      division; the sum over them of the eleven terms of step 3b under these centroids; steps 3c to 3e give h'.  h'
 *      INVALID: stop.  c' = the members under h'; c' < c: stop.  Otherwise h = h', c = c'.  Then
 *      rms = sqrtf(E / (float)c), E the sum of E2 over the members under h.  Every sum over members is the sum of
 *      misift_improve_fundamental_batch over the candidate position p: 256 partial sums from +0, slot p mod 256 adding
 *      its members in ascending p (a candidate that is no member adds nothing), then p[t] = p[t] + p[t + off] for
 *      off = 128 .. 1.  Status 0; d_align_inliers[e] = c; d_sim[16e .. 16e+15] = R row-major, t, s, rms, 0, 0.
 *   d_align_status[e] = the status.  d_inlier, when given: d_inlier[src_first + i] for every i < src_cap = 1 for a member
 *   under the final h of a status-0 entry, 0 for any other candidate, -1 for a source point that is no candidate.
 *   d_summary (8 ints, integer sums, so deterministic): [0] entries with status 0, [1] their inliers, [2] entries with
 *   status 1, [3] with status 2, [4] the candidates of all entries, [5] the refits kept, [6..7] 0.
 *   Every other byte stays untouched.
 *   - NULL ctx, d_src, d_dst, d_map, d_sim, d_align_cand, d_align_inliers, d_align_status or d_summary; nsel < 0, nsel > 0
 *     with NULL ranges or seeds; src_first or dst_first < 0, src_cap or dst_cap < 1, first + cap beyond 2^31 - 1;
 *     d_count given with count_stride < 0; num_loops < 1; thresh NaN or <= 0; min_inliers < 3; refit_loops < 0; d_inlier
 *     given and two entries' source ranges overlapping; nsel x ceil(num_loops / 64) x ceil(max src_cap / 512) beyond
 *     2^31 - 1 (one launch), or num_loops or a src_cap beyond 2^31 - 16: MISIFT_EINVAL, before anything is enqueued.
 *     nsel == 0 is no error: only d_summary is written.  None of the inputs is written.
 *   - Stream semantics as misift_resect_cameras_batch: `ranges` and `seeds` are copied; no host synchronisation and no
 *     host read.
 *   - One memset and five launches whatever the data: per entry the ordered candidate list and the draw, one lane per
 *     (entry, hypothesis) for the solve, one 64-lane workgroup per (entry, 64 hypotheses, 512 candidates) for the count
 *     (VALU work; the matrix cores' fused accumulation would break the definition), the pick, and one 256-thread
 *     workgroup per entry for the refit.  Temp memory from the library's own allocator, sized from nsel, the largest
 *     src_cap and num_loops only: per entry 28 bytes per candidate of the largest src_cap and 68 bytes per hypothesis
 *     (both rounded up to 16), and 80 bytes. */
int misift_align_points_batch(misift_ctx *ctx,
                              const float *d_src,             /* pooled, 4 floats per point */
                              const int *d_src_status,        /* pooled with d_src, may be NULL */
                              const float *d_dst,
                              const int *d_dst_status,        /* may be NULL */
                              const int *d_map,               /* pooled with d_src */
                              int nsel, const int *ranges,    /* host, nsel x 4, copied */
                              const unsigned *seeds,          /* host, nsel, copied */
                              const int *d_count, int count_stride,   /* may be NULL */
                              int num_loops, float thresh /* d_dst units */, int min_inliers, int refit_loops,
                              float *d_sim,                   /* nsel x 16 */
                              int   *d_align_cand,            /* nsel */
                              int   *d_align_inliers,         /* nsel */
                              int   *d_align_status,          /* nsel */
                              int   *d_inlier,                /* pooled with d_src, may be NULL */
                              int   *d_summary);              /* 8 ints */

/* misift_transform_scene_batch: the transform d_sim[0 .. 12] = R row-major, t, s (one entry of d_sim above) applied to
 * the points and the cameras of a scene, so that every reprojection is unchanged.  APPLY iff d_sim_status is NULL or
 * d_sim_status[0] == 0, read on the device.  T = min(max(d_export_summary[2], 0), max_tracks).
 *   Point t < max_tracks: with APPLY, t < T and d_point_status[t] == 0,
 *   d_points_out[4t + r] = s * ((R[r][0]*X_0 + R[r][1]*X_1) + R[r][2]*X_2) + t_r and the fourth word copied; otherwise
 *   all four words are copied bit for bit.
 *   Image i < nimages: with APPLY and d_cam_pair[i] != -2, from its R_i row-major and t_i:
 *   R'[r][c] = (R_i[r][0]*R[c][0] + R_i[r][1]*R[c][1]) + R_i[r][2]*R[c][2] (R' = R_i R^T),
 *   t'_r = s * t_i[r] - ((R'[r][0]*t_0 + R'[r][1]*t_1) + R'[r][2]*t_2): the camera frame scales with the world.
 *   Otherwise the twelve words are copied bit for bit.  A computed NaN is stored as 0x7fc00000.
 *   d_points_out may be d_points and d_cam_out may be d_cam; otherwise they share no byte.
 *   - NULL ctx or pointer other than d_sim_status; max_tracks or nimages < 1; an output that overlaps its input without
 *     being it: MISIFT_EINVAL, before anything is enqueued.  One launch, no temp, no host read. */
int misift_transform_scene_batch(misift_ctx *ctx,
                                 const float *d_sim,          /* 16 floats: one entry of misift_align_points_batch */
                                 const int *d_sim_status,     /* its status word, may be NULL */
                                 int max_tracks, const int *d_export_summary,
                                 const float *d_points,       /* max_tracks x 4 */
                                 const int *d_point_status,   /* max_tracks */
                                 int nimages,
                                 const float *d_cam,          /* nimages x 12 */
                                 const int *d_cam_pair,       /* nimages */
                                 float *d_points_out,         /* max_tracks x 4 */
                                 float *d_cam_out);           /* nimages x 12 */

/* misift_merge_scenes_batch: two exported scenes that lie in one gauge written out as ONE scene (no reference
 * counterpart): one export, one point array, one camera array and one record index, which triangulate, refine, resect,
 * filter and adjust take unchanged.  Scene B is the reference: its gauge is the merged gauge, and
 * misift_align_points_batch with A as the source and B as the destination followed by misift_transform_scene_batch on A
 * puts A's points and cameras there; this call takes A after that transform.  The chain
 * export A, export B -> triangulate each -> correspond -> align -> transform(A) -> merge(A into B) -> triangulate or
 * adjust on the merged scene runs with no host read.
 *   Per scene S (A or B): d_track_offsets_S, d_obs_S and d_export_summary_S from export (or filter) for max_tracks_S and
 *   max_obs_S; d_points_S, d_point_views_S and d_point_status_S from triangulate (A's points after the transform); d_cam_S
 *   and d_cam_pair_S for nimages_S images; d_record_obs_S (max_records_S ints, from export; read only when
 *   d_record_obs_out is given, otherwise it may be NULL and max_records_S is not looked at).  d_map (max_tracks_a ints) is
 *   what misift_correspond_tracks_batch wrote for (A, B); d_accept (max_tracks_a ints, may be NULL) is d_inlier of
 *   misift_align_points_batch for the entry whose source points are A's tracks.  Image i of S is image i + fshift_S of
 *   the merged scene, which has nimages_out images; global record g of S is record g + rshift_S of the merged index of
 *   max_records_out records.  rshift_b - rshift_a is the `shift` correspond was called with; the call does not check
 *   that.  Intrinsics are host arrays: the caller lays out the merged scene's itself.
 *   T_A, O_A, T_B and O_B are read on the device and clamped as in misift_correspond_tracks_batch.  VALID tracks and the
 *   OWNER of a slot are those of misift_refine_cameras_batch, per scene; the observations of a valid track are the slots
 *   it owns.  Everything is integer work and bit copies: there is no floating-point arithmetic in the call.
 *   1. Live observations.  Slot o of a valid track of scene S is LIVE iff its frame lies in [0, nimages_S).  Its KEY is
 *      the 64-bit value ((int64)(frame + fshift_S) << 32) | (uint32)record.
 *   2. Class of A-track t < T_A, the first that applies: -1 the track is not valid; -2 d_map[t] == -2; -4 d_map[t] < -2
 *      or d_map[t] >= T_B; -3 d_map[t] >= 0, d_accept is given and d_accept[t] == 0 (a tie that the 3-D test rejected).
 *      Otherwise the track is a PARTNER of B-track d_map[t] when that is >= 0 and ALONE when it is -1.  A tie whose
 *      d_accept is 1 or -1 is merged (-1: one of the two points failed, so nothing speaks against the shared records).
 *   3. Merged tracks.  B-track tB < T_B is merged track t' = tB: B's numbering is kept.  The ALONE A-tracks follow in
 *      ascending tA: t' = T_B + the number of ALONE tracks before tA; N = T_B + the number of ALONE tracks.  The UNION of
 *      t' < T_B is the live observations of tB (source 0; none if tB is not valid) and the live observations of every
 *      PARTNER of tB (source 1); the UNION of an ALONE track is its own live observations (source 1).  An element of a
 *      union is KEPT iff no other element of that union has the same KEY and a smaller (source, slot): a record seen by
 *      both scenes stays once, as B's, and hostile duplicates inside one list collapse too.  len'[t'] = the number of
 *      kept elements; a kept element's place in the track = the number of kept elements with a smaller KEY (ascending
 *      (frame, record): export's order for any layout whose frames ascend in memory).  Both rules are order-free, so the
 *      output depends neither on the order in which partners are enumerated (the partner lists are filled by atomicAdd,
 *      unordered) nor on whether the input lists are sorted.  len' == 0 is allowed and keeps its number.
 *   4. Capacity, as export's.  off'[t'] = the sum of len' before t' (in 64 bits).  Track t' is WRITTEN iff
 *      t' < max_tracks_out and off'[t'] + len'[t'] <= max_obs_out.  The written tracks are a prefix T' holding O'
 *      observations; no track is cut in the middle.
 *   5. Outputs, for t' < T': d_track_offsets_out[0 .. T'] = off' ([0] = 0 always); d_obs_out[off' + k] = for the k-th
 *      kept element its frame + fshift_S, its record, and the bits of xpos and ypos; d_points_out[4t' .. 4t'+3],
 *      d_point_views_out[t'] and d_point_status_out[t'] = bit copies from B at tB when t' < T_B and from A at tA otherwise
 *      (the rms word and the view count are stale by construction: call triangulate or adjust next).
 *      d_track_map_a[t], t < T_A: the negative class, or the merged t', or -6 when that t' >= T'.
 *      d_obs_map_a[o], o < O_A (may be NULL): -1 when the slot has no owner; the owner's negative code (its class, or -6)
 *      when the owner was dropped or cut; -5 when the observation is not live; otherwise the new slot of the kept element
 *      with its KEY, so a duplicate maps onto its surviving twin.  d_obs_map_b[o], o < O_B (may be NULL): the same, with
 *      -1, -6, -5 or the slot.
 *      d_record_obs_out (max_records_out ints, may be NULL; needs both d_record_obs_a and d_record_obs_b): every entry is
 *      written.  Entry g' = the first that applies: d_obs_map_b[d_record_obs_b[g' - rshift_b]] when the index lies in
 *      [0, max_records_b), the slot in [0, O_B) and the map value is >= 0; else the same through A; else -1 (the map
 *      values are those defined above whether or not the maps are given).
 *      Cameras, image i' < nimages_out, the first that applies: iB = i' - fshift_b lies in [0, nimages_b) and
 *      d_cam_pair_b[iB] != -2: B's twelve words bit for bit and d_cam_pair_out[i'] = d_cam_pair_b[iB]; the same holds
 *      through A: A's twelve words and d_cam_pair_out[i'] = MISIFT_CAM_MERGED (a second root must not appear; as stated
 *      under misift_resect_cameras_batch every value but -2 means "has a camera" and only -1 is the root); neither:
 *      twelve zeros and -2.
 *      d_export_summary_out (export's layout): [0] N, [1] the kept observations of all N tracks, [2] T', [3] O', [4] the
 *      longest written track, [5..7] 0.  d_summary (8 ints): [0] T', [1] O', [2] A-tracks written as partners, [3]
 *      A-tracks written alone, [4] A-tracks with class -1 ... -4, [5] duplicate observations removed in written tracks,
 *      [6] N - T', [7] images whose camera came from A.
 *      Outputs beyond T', T' + 1 (the offsets), O', T_A (d_track_map_a), O_A and O_B (the slot maps) stay untouched.
 *   - Not done here: B's point is taken as it is and the merged point is not re-estimated (triangulate or adjust does
 *     that next); an A-track tied to several B-tracks (-2) is dropped, not used to join them; intrinsics are the caller's.
 *   - NULL ctx, or a NULL pointer other than d_accept, d_obs_map_a, d_obs_map_b and d_record_obs_out (and the two
 *     d_record_obs_S without it); a capacity or image count < 1 (max_records_* only with d_record_obs_out); a negative
 *     shift; nimages_S + fshift_S > nimages_out, or max_records_S + rshift_S > max_records_out where d_record_obs_out is
 *     given; d_record_obs_out given without both input record arrays; d_obs_a, d_obs_b or d_obs_out not 16-byte aligned;
 *     any output overlapping an input or another output, each at its stated size: MISIFT_EINVAL, before anything is
 *     enqueued.  None of the inputs is written.
 *   - Deterministic: byte-identical from run to run.  Every index read from device memory (T, O, offsets, frames, map
 *     values, record slots) is range-checked before it addresses anything.
 *   - The call runs on the context stream and returns before the GPU work is done; no host synchronisation and no host
 *     read.  Ordering behind batches in flight (K > 1): as misift_match_batch.
 *   - Three memsets and ten launches whatever the data: the owners of both scenes, one lane per A-track for the class and
 *     the partner counts, the scan of 2048-track tile sums in one workgroup and one lane per B-track for the partner
 *     lists, their unordered fill, one wavefront per merged track for the union (its first 256 elements staged on chip,
 *     ranked by all-pairs comparison across the 64 lanes; a longer union takes a piece of temp memory), the tile scan and
 *     one lane per merged track for the numbering, and one lane per slot, A-track, record and image for the copy.  No
 *     workgroup waits for another.  Temp memory from the library's own allocator, sized from the capacities only: 24
 *     bytes per slot of max_obs_a + max_obs_b, 20 per track of max_tracks_a, 20 per track of max_tracks_b plus 16 per
 *     2048 tracks, each array rounded up to 16. */
#define MISIFT_CAM_MERGED (-4)
int misift_merge_scenes_batch(misift_ctx *ctx,
                              int max_tracks_a, int max_obs_a,
                              const int *d_track_offsets_a,     /* max_tracks_a + 1, from export */
                              const misift_track_obs *d_obs_a,  /* max_obs_a, 16-byte aligned */
                              const int *d_export_summary_a,    /* 8 ints: [2] = T_A, [3] = O_A */
                              const float *d_points_a,          /* max_tracks_a x 4, after the transform */
                              const int *d_point_views_a,       /* max_tracks_a */
                              const int *d_point_status_a,      /* max_tracks_a */
                              int nimages_a,
                              const float *d_cam_a,             /* nimages_a x 12, after the transform */
                              const int *d_cam_pair_a,          /* nimages_a */
                              int max_records_a, const int *d_record_obs_a,   /* may be NULL */
                              int max_tracks_b, int max_obs_b,
                              const int *d_track_offsets_b, const misift_track_obs *d_obs_b,
                              const int *d_export_summary_b, const float *d_points_b, const int *d_point_views_b,
                              const int *d_point_status_b, int nimages_b, const float *d_cam_b,
                              const int *d_cam_pair_b, int max_records_b, const int *d_record_obs_b,
                              const int *d_map,                 /* max_tracks_a, from correspond */
                              const int *d_accept,              /* max_tracks_a, d_inlier of align; may be NULL */
                              int fshift_a, int fshift_b, int nimages_out,
                              int rshift_a, int rshift_b, int max_records_out,
                              int max_tracks_out, int max_obs_out,
                              int *d_track_offsets_out,         /* max_tracks_out + 1 */
                              misift_track_obs *d_obs_out,      /* max_obs_out, 16-byte aligned */
                              int *d_export_summary_out,        /* 8 ints, export's layout */
                              float *d_points_out,              /* max_tracks_out x 4 */
                              int *d_point_views_out,           /* max_tracks_out */
                              int *d_point_status_out,          /* max_tracks_out */
                              float *d_cam_out,                 /* nimages_out x 12 */
                              int *d_cam_pair_out,              /* nimages_out */
                              int *d_track_map_a,               /* max_tracks_a: t', or the reason */
                              int *d_obs_map_a,                 /* max_obs_a: the new slot or the reason; may be NULL */
                              int *d_obs_map_b,                 /* max_obs_b; may be NULL */
                              int *d_record_obs_out,            /* max_records_out; may be NULL */
                              int *d_summary);                  /* 8 ints */

/* misift_describe_points_batch: an 8-bit descriptor per track point, laid out as a one-frame record set that the int8
 * pair matchers take (no reference counterpart).  With misift_localize_frames_batch below it places a frame that arrived
 * after the tracks were linked: quantize the new frames -> describe -> misift_match_pairs_batch_i8 (new frame, scene) ->
 * localize -> merge -> refine / adjust, with no host read.
 *   d_track_offsets, d_obs, d_export_summary: from export (or filter, or merge) for max_tracks and max_obs; d_points and
 *   d_point_status from triangulate.  d_q is what misift_quantize_batch wrote for the record batch the observations
 *   index: nframes frames, d_counts, d_offsets or stride, max_records records in all.  The layout and the rule "a frame
 *   whose records do not all lie in [0, max_records) takes no part" are those of misift_link_tracks_batch:
 *   n(f) = max(d_counts[f], 0), base(f) = d_offsets[f], or f * stride without d_offsets (in 64 bits); frame f TAKES PART
 *   iff n(f) == 0 or 0 <= base(f) and base(f) + n(f) <= max_records.
 *   T and O are read on the device and clamped as in misift_refine_cameras_batch: T = min(max(d_export_summary[2], 0),
 *   max_tracks), O likewise with [3] and max_obs.  Track t < T is VALID by the rule of misift_refine_cameras_batch:
 *   0 <= off[t] <= off[t+1] <= O.  The observations of a valid track are the slots off[t] .. off[t+1] - 1, its own range
 *   whether or not another track's range overlaps it (the call only reads: there is no owner rule); a track that is not
 *   valid has none.
 *   An observation (frame f, record r) CONTRIBUTES iff f lies in [0, nframes), frame f takes part and r lies in
 *   [0, n(f)).  Its descriptor row is the 128 signed bytes at d_q + 128 * (base(f) + r).  xpos and ypos are not read.
 *   Per track t < T: m = the number of its contributing observations; sum_k = the sum of byte k over them, as integers
 *   (the library sums in 64 bits).  The point is DESCRIBED iff the track is valid, d_point_status[t] == 0, d_points[4t],
 *   [4t+1] and [4t+2] are FINITE (fabsf(v) <= FLT_MAX) and m > 0.  A described point has byte k =
 *   (2 * sum_k + m) / (2 * m) in integer division: the mean, a half rounded up, in [0, 127] for the bytes quantize writes.
 *   Outputs, for t < T (what lies at or beyond T stays untouched):
 *     d_scene_q[128t .. 128t+127]   the bytes of a described point; 128 zeros otherwise.  Every int8 matcher counts only
 *                                   S > 0, so a zero row is nobody's match and nobody's second best: no compaction.
 *     d_scene_recs record t         every one of its 576 bytes: zeros, except that a described point has the bits of X, Y, Z
 *                                   in xpos, ypos, scale.  The pair matcher copies xpos / ypos of set 2, so match_xpos and
 *                                   match_ypos of a row carry X and Y.
 *     d_point_members[t]            m.
 *   d_scene_count[0] = T.  d_summary (8 ints, integer sums, so deterministic): [0] T, [1] described points, [2] the
 *   contributing observations of described points, [3] observations of valid tracks that do not contribute (an
 *   observation in the ranges of two tracks counts with each), [4..7] 0.
 *   The scene then is set 2 of misift_match_pairs_batch_i8 as ONE frame: d_recs2 = d_scene_recs, d_q2 = d_scene_q,
 *   nframes2 = 1, d_counts2 = d_scene_count, d_offsets2 = NULL, stride2 = max_tracks, pairs (query frame, 0).  `match` of
 *   a row is the track number.  That call turns a pair away whose set-2 frame holds more than its max_pts records, so
 *   its max_pts is at least T (max_tracks always does), and so is the stride of its output rows; the max_pts of
 *   misift_localize_frames_batch is its own and bounds the rows of a query frame only.
 *   - Not done here: the mean is not renormalised, so scores against points are lower than cosines (the ambiguity ratio
 *     is unaffected; min_score is the caller's); no fp32 descriptor: `data` of the scene records is zero and the fp32
 *     matchers find nothing there.
 *   - NULL ctx or pointer other than d_offsets; max_tracks, max_obs or max_records < 1; nframes < 0; d_offsets NULL with
 *     stride < 0; d_obs, d_q, d_scene_q or d_scene_recs not 16-byte aligned; an output that shares a byte with an input or
 *     with another output, each at its stated size (d_q: 128 * max_records bytes, d_counts and d_offsets: nframes ints):
 *     MISIFT_EINVAL, before anything is enqueued.  None of the inputs is written.
 *   - Integer work only and deterministic: byte-identical from run to run whatever the dispatch order.  Every index read
 *     from device memory (T, O, offsets, frames, records, counts, frame offsets) is range-checked before it addresses
 *     anything.
 *   - The call runs on the context stream and returns before the GPU work is done; no host synchronisation and no host
 *     read.  Ordering behind batches in flight (K > 1): as misift_match_batch.
 *   - One memset and one launch: one wavefront per track, 16 lanes per observation with 8 bytes of its row each.  No temp
 *     memory. */
int misift_describe_points_batch(misift_ctx *ctx,
                                 int max_tracks, int max_obs,
                                 const int *d_track_offsets,     /* max_tracks + 1, from export */
                                 const misift_track_obs *d_obs,  /* max_obs, from export, 16-byte aligned */
                                 const int *d_export_summary,    /* 8 ints, from export: [2] = T, [3] = O */
                                 const float *d_points,          /* max_tracks x 4, from triangulate */
                                 const int *d_point_status,      /* max_tracks, from triangulate */
                                 const void *d_q,                /* max_records x 128 int8, from quantize, 16-byte aligned */
                                 int nframes, const int *d_counts, const int *d_offsets, int stride,
                                 int max_records,
                                 void *d_scene_q,                /* max_tracks x 128 int8, 16-byte aligned */
                                 void *d_scene_recs,             /* max_tracks records of 576 bytes, 16-byte aligned */
                                 int *d_scene_count,             /* 1 int */
                                 int *d_point_members,           /* max_tracks */
                                 int *d_summary);                /* 8 ints */

/* misift_localize_frames_batch: the camera of a new image from the rows of a frame matched against the scene's points,
 * by the search of misift_resect_cameras_batch over 2-D/3-D matches, and the inliers written out as a scene that
 * misift_merge_scenes_batch takes as its scene A (no reference counterpart).  Resect finds its candidates through d_obs,
 * so it places only images whose records sit in the exported tracks; here the candidates come from match rows.
 *   The rows are a batch as misift_find_homography_batch takes it: d_rows, nframes_rows frames, d_counts, d_offsets or
 *   stride.  After misift_match_pairs_batch_i8: frame i = pair i, stride = its max_pts, d_counts = d_out_counts.
 *   d_export_summary, d_points, d_point_status: the scene's, for max_tracks; T as in misift_describe_points_batch.
 *   intrinsics[4i..4i+3] = fx fy cx cy of image i < nimages.  Entry e < nsel works on the rows of frame frames[e], gives
 *   the camera of image images[e] (distinct; so are the frames) with the seed seeds[e], and writes result slot e.
 *   The arithmetic, FINITE and the NaN rule are those of misift_resect_cameras_batch.
 *   Per entry e, independently of every other entry:
 *   1. Skip: step 1 of misift_resect_cameras_batch with i = images[e] (status 3).
 *   2. Candidates.  c = d_counts[frames[e]].  c > max_pts: status 4, d_res_cand[e] = 0, twelve zeros, d_res_inliers[e] = 0
 *      and nothing of the frame is read.  Otherwise the frame has max(c, 0) rows, and row r is a CANDIDATE, in ascending
 *      r, iff score > min_score and ambiguity < max_ambiguity (a NaN fails); t = match lies in [0, T);
 *      d_point_status[t] == 0; d_points[4t], [4t+1], [4t+2] are FINITE; xpos and ypos are FINITE.  Candidate p < n has
 *      (x, y) = the row's xpos, ypos and (X, Y, Z) = d_points[4t..4t+2].  d_res_cand[e] = n.  n < max(6, min_inliers):
 *      status 1, twelve zeros and d_res_inliers[e] = 0.
 *   3. Draw, solve, count, pick and install: steps 3 to 7 of misift_resect_cameras_batch, word for word, under the
 *      intrinsics of image images[e]; d_cam and d_cam_pair are indexed by images[e].
 *   4. Emit.  A FIND is a candidate of an entry with status 0 that is an inlier (step 5) of the entry's picked hypothesis,
 *      tested on the hypothesis as the count tested it; an entry has exactly d_res_inliers[e] finds.  The finds are
 *      numbered a = 0, 1, ... over the entries in ascending e and within an entry in ascending r; N = their number.  Find
 *      a is WRITTEN iff a < max_found; T' = min(N, max_found).  For a written find of entry e from row r naming point t:
 *      d_found_offsets[a] = a; d_found_obs[a] = (frame images[e], record r, the bits of x and y); d_found_map[a] = t;
 *      d_found_points[4a..4a+3] = bit copies of d_points[4t..4t+3]; d_found_views[a] = 1; d_found_status[a] = 0.
 *      d_found_offsets[T'] = T' closes the last track.  d_found_summary (export's layout): [0] N, [1] N, [2] T', [3] T',
 *      [4] 1 if T' > 0 else 0, [5..7] 0.  What lies at or beyond T' (T' + 1 for the offsets) stays untouched.
 *      Two rows of one frame that name the same point are two finds; misift_filter_tracks_batch with unique_frames
 *      resolves them after the merge.
 *   d_res_cam, d_res_cand, d_res_inliers, d_res_status and d_summary[0..6] are as in misift_resect_cameras_batch;
 *   d_summary[7] = T'.
 *   The merge then needs nothing more: with install the localised cameras are in the caller's d_cam at images[e] (sized
 *   to hold the new images, which start at d_cam_pair == -2); d_found_* is scene A with max_tracks_a = max_obs_a =
 *   max_found and d_found_map is d_map; d_accept NULL, fshift 0 and the same camera arrays on both sides.
 *   - Not done here: no guided second pass against projected points; no P3P solver and no local optimisation inside the
 *     search (as resect); the pairs of the match are the caller's host list, not device data.
 *   - NULL ctx; NULL d_rows, d_counts, d_export_summary, d_points, d_point_status, intrinsics, d_res_*, d_summary or
 *     d_found_*; d_offsets NULL with stride < 0; max_tracks, nimages, nframes_rows, max_pts or max_found < 1; NULL
 *     d_cam_pair with only_unset or install set, NULL d_cam with install set; d_found_obs not 16-byte aligned; nsel < 0,
 *     nsel > 0 with NULL frames, images or seeds; a frame outside [0, nframes_rows) or an image outside [0, nimages) or
 *     either listed twice; num_loops < 1; min_inliers < 6; min_score or max_ambiguity NaN; thresh NaN or <= 0;
 *     only_unset or install other than 0 or 1; intrinsics as in misift_resect_cameras_batch; nsel x ceil(num_loops / 64)
 *     x ceil(max_pts / 512) beyond 2^31 - 1 (one launch), or num_loops or max_pts beyond 2^31 - 16: MISIFT_EINVAL, before
 *     anything is enqueued.  nsel == 0 is no error: only d_summary, d_found_summary and d_found_offsets[0] are written.
 *     None of the inputs is written, except d_cam and d_cam_pair under install.
 *   - Deterministic: the base of an entry's finds is an integer prefix over the entries before it.
 *   - The call runs on the context stream and returns before the GPU work is done; the host lists are copied; no host
 *     synchronisation and no host read.  Ordering behind batches in flight (K > 1): as misift_match_batch.
 *   - One memset and five launches whatever the data (nsel == 0: the memset and two launches): per entry the ordered
 *     candidate list and the draw, resect's solve and count, the pick, and per entry the ordered list of finds.  Temp
 *     memory from the library's own allocator, sized from nsel, max_pts and num_loops only: per entry 24 bytes per row of
 *     max_pts and 76 bytes per hypothesis (both rounded up to 16), and 24 bytes. */
int misift_localize_frames_batch(misift_ctx *ctx,
                                 const void *d_rows, int nframes_rows, const int *d_counts, const int *d_offsets,
                                 int stride,
                                 int max_tracks,
                                 const int *d_export_summary,    /* 8 ints: [2] = T */
                                 const float *d_points,          /* max_tracks x 4 */
                                 const int *d_point_status,      /* max_tracks */
                                 int nimages,
                                 const float *intrinsics,        /* host, nimages x 4: fx fy cx cy, copied */
                                 int nsel, const int *frames,    /* host, nsel distinct frames of the rows, copied */
                                 const int *images,              /* host, nsel distinct image indices, copied */
                                 const unsigned *seeds,          /* host, nsel, copied */
                                 int max_pts, float min_score, float max_ambiguity,
                                 int num_loops, float thresh /* px */, int min_inliers, int only_unset, int install,
                                 float *d_cam,                   /* nimages x 12: written when install */
                                 int   *d_cam_pair,              /* nimages: read when only_unset, written when install */
                                 float *d_res_cam,               /* nsel x 12 */
                                 int   *d_res_cand,              /* nsel */
                                 int   *d_res_inliers,           /* nsel */
                                 int   *d_res_status,            /* nsel */
                                 int   *d_summary,               /* 8 ints */
                                 int max_found,
                                 int *d_found_offsets,           /* max_found + 1 */
                                 misift_track_obs *d_found_obs,  /* max_found, 16-byte aligned */
                                 int *d_found_summary,           /* 8 ints, export's layout */
                                 float *d_found_points,          /* max_found x 4 */
                                 int *d_found_views,             /* max_found */
                                 int *d_found_status,            /* max_found */
                                 int *d_found_map);              /* max_found */

/* The cameras and the track points adjusted jointly (bundle adjustment; no reference counterpart): what
 * misift_refine_cameras_batch and misift_triangulate_tracks_batch do in turns, done in one Levenberg-Marquardt step over
 * all free cameras (6 parameters each) and all active track points (3 each).  Each step eliminates the points (Schur
 * complement), solves the reduced camera system matrix-free by cg_iters block-Jacobi preconditioned conjugate-gradient
 * iterations, back-substitutes the points, and is kept or turned away on the device.  In the chain: ... export ->
 * triangulate -> resect -> triangulate -> refine -> adjust.
 *   The inputs are those of misift_refine_cameras_batch, read the same way; d_points[4t+3] and obs.record are not read.
 *   The arithmetic is that of misift_refine_cameras_batch: fp32, every operation rounded, only + - * / sqrtf and fabsf,
 *   no contraction, a comparison with a NaN is false, everything taken left to right as written.  a . b of two
 *   6-vectors is ((((a0*b0 + a1*b1) + a2*b2) + a3*b3) + a4*b4) + a5*b5.
 *   T, O, valid tracks, the OWNER of a slot and the CANDIDATES of an image are those of misift_refine_cameras_batch.
 *   Sets, decided once under the starting cameras and points:
 *   - Image i has NO CAMERA (status 4) iff d_cam_pair[i] == -2 or one of its twelve floats is not finite; otherwise it is
 *     HELD (status 3) iff d_cam_pair[i] == -1 or i is in `hold`; otherwise it is FREE.  With orthonormalise == 1 a free
 *     camera goes through step 1 of misift_refine_cameras_batch first; a non-finite result makes it status 4 (its
 *     twelve floats as given).  An image is USABLE iff its status is not 4.
 *   - A candidate is a PRE-MEMBER iff its image is usable and the member test of misift_refine_cameras_batch holds under
 *     that camera: Xc.z > 0 and ru*ru + rv*rv < E2, E2 = max_error*max_error rounded once on the host (+inf: in front
 *     alone).  A valid track is ACTIVE iff it owns at least min_views pre-members.  The MEMBERS are the pre-members of
 *     active tracks; the set does not change afterwards.  n_i = the members of image i, n_t = those of track t.
 *   - A free image with n_i < min_obs is demoted: status 1, its camera (of step 1) constant.  There is no cascade: its
 *     members, like those of held images, still constrain their points.  That is how held cameras fix the gauge.
 *   Sums.  A PER-TRACK sum runs over the track's members in ascending slot, from +0, one term at a time.  A PER-IMAGE
 *   sum runs over the image's members listed in ascending slot, by the 256-slot rule of
 *   misift_improve_fundamental_batch on the position in that list: p[s], s < 256, starts at +0 and adds the terms of
 *   positions s, s + 256, ... in ascending order; then for off = 128 ... 1: p[s] = p[s] + p[s + off] for s < off; the sum
 *   is p[0].  A CROSS-IMAGE sum is the same rule on the image index; an image that does not take part is skipped.
 *   The COST of a state (cameras, points): per member, Xc, iz, a, b, ru, rv as in step 2 of
 *   misift_refine_cameras_batch; the image's cost c_i is the per-image sum of ru*ru + rv*rv, and c the cross-image sum
 *   of c_i over all images.  A state with a member whose Xc.z > 0 is false is NOT IN FRONT.
 *   One LM step at damping lambda (lambda = lambda0 at first), l1 = 1 + lambda:
 *   1. Per member under the state: Ju, Jv (camera, 6 each) as step 3 of misift_refine_cameras_batch; the point's
 *      Pu = gx * (r0 - a*r2), Pv = gy * (r1 - b*r2) per component with gx = fx*iz, gy = fy*iz;
 *      W[r][q] = Ju[r]*Pu[q] + Jv[r]*Pv[q].  (W v)[r] = (W[r][0]*v0 + W[r][1]*v1) + W[r][2]*v2 for a 3-vector v and
 *      (W^T v)[q] = ((((W[0][q]*v0 + W[1][q]*v1) + W[2][q]*v2) + W[3][q]*v3) + W[4][q]*v4) + W[5][q]*v5 for a 6-vector.
 *   2. Per active track, per-track sums in the order of step 3 of misift_triangulate_tracks_batch (the row Pu with rhs
 *      ru, then the row Pv with rhs rv): V (M00 M01 M02 M11 M12 M22) and gp.  V' = V with M00, M11, M22 each multiplied
 *      by l1.  y_t = SOLVE(V', gp) of misift_triangulate_tracks_batch.
 *   3. Per free image, 33 per-image sums: U[r][q], r <= q, with the term Ju[r]*Ju[q] + Jv[r]*Jv[q]; gc[r] with
 *      Ju[r]*ru + Jv[r]*rv; s[r] with (W y_t)[r], t the member's track.  U' = U with each diagonal entry multiplied by
 *      l1; b[r] = gc[r] - s[r].  M^-1 v is the SOLVE of step 4 of misift_refine_cameras_batch with U' and v.
 *      A SOLVE of step 2 or 3 that fails (a pivot that is not finite and > 0, a result that is not finite; step 3 checks
 *      M^-1 b) makes the step FAIL: nothing below is computed, c' is the quiet NaN and the CG iterations are 0.
 *   4. PCG over the free images.  x = 0, r = b, z = M^-1 r, p = z, rho = the cross-image sum of r_i . z_i; rho not
 *      finite: no iteration runs.  Then cg_iters times at the most:
 *        per active track q_t = SOLVE(V', the per-track sum of (W^T p_i) over its members in free images);
 *        per free image y_i[r] = U'[r] . p_i - (the per-image sum of (W q_t)[r]);
 *        sigma = the cross-image sum of p_i . y_i; unless sigma is finite and > 0, CG ends here with x as it stands;
 *        alpha = rho / sigma; x += alpha*p, r -= alpha*y per component; z = M^-1 r; rho' = the cross-image sum of
 *        r_i . z_i; the iteration counts; rho' not finite: CG ends here; beta = rho' / rho, p = z + beta*p, rho = rho'.
 *      A SOLVE or M^-1 whose result is not finite gives zeros.  cg_iters == 0 or no free image leaves x = 0: the step
 *      then moves the points only.
 *   5. Per active track delta_t = SOLVE(V', gp - the per-track sum of (W^T x_i) over its members in free images),
 *      X' = X + delta_t per component; per free image the Cayley update of step 5 of misift_refine_cameras_batch with
 *      x_i.
 *   6. c' = the cost of the trial state.  The step is KEPT iff it did not fail, every trial camera and point is finite,
 *      the trial state is in front and c' < c.  Kept: the trial state becomes the state, lambda <- max(lambda / 10, 1e-7).
 *      Otherwise the state stays and lambda <- 10 * lambda: the raised lambda is the retry, so, unlike
 *      misift_refine_cameras_batch, the loop does not end there.  All num_loops steps are always enqueued.
 *      d_history[4k..4k+3] of step k: c' (the quiet NaN unless the trial state is finite and in front), the lambda used,
 *      1 if kept else 0 (int), the CG iterations that counted (int).
 *   Outputs.  d_cam_out[12i..]: the camera of the final state for a free or demoted image, the twelve input floats bit
 *   for bit for any other.  d_cam_obs[i] = n_i; d_cam_status[i] = 0 adjusted (free), 1 demoted, 3 held or root, 4 no
 *   camera; d_cam_rms[2i], [2i + 1] = sqrtf(c_i / (float)n_i) under the starting and the final state (the quiet NaN when
 *   n_i == 0).  For t < T: d_point_obs[t] = the pre-members track t owns (0 for a track that is not valid); an active
 *   track gets d_points_out[4t..4t+2] = its point of the final state and [4t+3] = sqrtf(ct / (float)n_t), ct the
 *   per-track sum of ru*ru + rv*rv; every other track t < T gets its four input words bit for bit.  Entries at or beyond
 *   T stay untouched.  d_cost[0], [1] = c of the starting and of the final state.  d_summary (8 ints, integer sums):
 *   [0] T, [1] images with status 0, [2] members, [3] images with status 1, [4] active tracks, [5] images with status 3,
 *   [6] steps kept, [7] images with status 4.  A single result that is a NaN is stored as 0x7fc00000.
 *   - With num_loops == 0 and orthonormalise == 0 every camera and point comes back bit for bit, and d_cost[0] ==
 *     d_cost[1].  On planted scenes with 0.5 px noise the fp32 result stays within the figures of
 *     tests/test_bundle_cpu.py (MEASURED) of the same algorithm in float64.
 *   - Departures from a textbook statement: the cost of a state is evaluated in a pass of its own (per slot, then per
 *     image), not with the linearisation, so that num_loops == 0 and the trial evaluation share one code path; the
 *     preconditioner is the damped U' of each camera, not the Schur diagonal block.
 *   - Not done here: no robust kernel re-weights a residual in this call (max_error is a hard gate, decided once:
 *     misift_adjust_bundle_robust_batch is this call under a Huber or a Geman-McClure loss), the intrinsics are not
 *     refined (misift_adjust_bundle_focal_batch refines a focal scale per camera), the member set is not revised
 *     between steps, and no Schur-diagonal preconditioner is formed.
 *   - NULL ctx; max_tracks, max_obs or nimages < 1; NULL d_track_offsets, d_obs, d_export_summary, d_points,
 *     d_point_status, d_cam, d_cam_pair, intrinsics, d_cam_out, d_points_out, d_cam_obs, d_cam_status, d_cam_rms,
 *     d_point_obs, d_cost or d_summary, NULL d_history with num_loops > 0; d_obs not 16-byte aligned; min_views < 2;
 *     min_obs < 3; num_loops < 0; cg_iters < 0; max_error NaN or <= 0; lambda0 not finite or <= 0; orthonormalise other
 *     than 0 or 1; nhold < 0, nhold > 0 with NULL hold, a hold index outside [0, nimages); an fx or fy that is not
 *     finite and > 0 or a cx or cy that is not finite; d_cam_out overlapping d_cam, or d_points_out overlapping
 *     d_points, without being equal to it: MISIFT_EINVAL, before anything is enqueued.  None of the inputs is written,
 *     except d_cam and d_points when they are the outputs.
 *   - The call runs on the context stream and returns before the GPU work is done; `intrinsics` and `hold` are copied;
 *     no host synchronisation and no host read.  Ordering behind batches in flight (K > 1): as misift_match_batch.
 *   - Three memsets and 11 + num_loops * (8 + 3 * cg_iters) launches whatever the data: per-track work one lane per
 *     track, per-image work one 256-thread workgroup per image (thread s = slot s of the sum), the cross-image scalars
 *     and the 6-vector updates in one workgroup; a dispatch boundary is the only barrier between workgroups.  Temp
 *     memory from the library's own allocator, sized from the capacities only: 100 bytes per slot, 76 per track and
 *     352 per image, each array rounded up to 16. */
int misift_adjust_bundle_batch(misift_ctx *ctx,
                               int max_tracks, int max_obs,
                               const int *d_track_offsets,     /* max_tracks + 1, from export */
                               const misift_track_obs *d_obs,  /* max_obs, from export, 16-byte aligned */
                               const int *d_export_summary,    /* 8 ints, from export: [2] = T, [3] = O */
                               const float *d_points,          /* max_tracks x 4, from triangulate */
                               const int *d_point_status,      /* max_tracks, from triangulate */
                               int nimages,
                               const float *d_cam,             /* nimages x 12 */
                               const int *d_cam_pair,          /* nimages */
                               const float *intrinsics,        /* host, nimages x 4: fx fy cx cy, copied */
                               int nhold, const int *hold,     /* host, images kept as they are, copied; may be NULL */
                               int min_views, int min_obs, int num_loops, int cg_iters,
                               float max_error, float lambda0, int orthonormalise,
                               float *d_cam_out,               /* nimages x 12; may be d_cam itself */
                               float *d_points_out,            /* max_tracks x 4; may be d_points itself */
                               int   *d_cam_obs,               /* nimages */
                               int   *d_cam_status,            /* nimages */
                               float *d_cam_rms,               /* nimages x 2: before, after */
                               int   *d_point_obs,             /* max_tracks */
                               float *d_history,               /* num_loops x 4 words */
                               float *d_cost,                  /* 2: before, after */
                               int   *d_summary);              /* 8 ints */

/* misift_adjust_bundle_batch under a robust loss (no reference counterpart): iteratively re-weighted least squares, the
 * weight of a member taken afresh from its residual under the state of every step.  Where the plain call minimises the
 * sum of ru*ru + rv*rv, this one minimises the sum of rho(ru*ru + rv*rv), so that an observation far off its point pulls
 * with a bounded (Huber) or a vanishing (Geman-McClure) force instead of a growing one, and nothing has to be removed
 * first.  In the chain it stands where adjust stands.
 *   The arguments are those of misift_adjust_bundle_batch in the same order, with `loss` and `loss_scale` after
 *   `orthonormalise` and `d_obs_weight` between `d_cost` and `d_summary`.  The definition is that of
 *   misift_adjust_bundle_batch, every word of it, the arithmetic rules included (fp32, every operation rounded, only
 *   + - * / sqrtf and fabsf, no contraction, a comparison with a NaN is false, left to right as written), with three
 *   amendments.
 *   The loss.  c = loss_scale, c2 = c*c rounded once on the host, s = ru*ru + rv*rv of a member.
 *     loss 0 (MISIFT_LOSS_NONE): rho = s, w = 1; the rows are not touched and loss_scale is not read.
 *     loss 1 (MISIFT_LOSS_HUBER): if s <= c2 then rho = s and w = sw = 1; otherwise (a NaN s too) n = sqrtf(s),
 *       rho = (c + c) * n - c2, w = c / n, sw = sqrtf(w).
 *     loss 2 (MISIFT_LOSS_GEMAN_MCCLURE): d = c2 + s, q = c2 / d, rho = (s * c2) / d, w = q * q, sw = q.
 *   Step 1.  The 20 values Ju, Jv (camera), Pu, Pv, ru, rv of a member are computed as there; s is taken from the
 *   unscaled ru, rv.  With loss != 0 each of the 20 values v then becomes sw * v, always, also when sw == 1.  Steps 2 to 5
 *   are unchanged and read the scaled values: W, V, gp, U, gc carry w = sw*sw through the products they are made of.
 *   There is no second-order (Triggs) correction.
 *   The cost.  Wherever that definition sums ru*ru + rv*rv it sums rho(s) instead: c_i, c, c' and the per-track ct.  The
 *   step is kept iff c' < c on that cost.  d_cam_rms[2i], [2i + 1] and d_points_out[4t+3] so become sqrtf of the mean
 *   rho, which is the rms reprojection error only with loss 0 (or while every member is a Huber inlier); d_cost and
 *   d_history[4k] are sums of rho.
 *   d_obs_weight, when not NULL, for o < O: -1.0f for a slot that is not a member; for a member, w under the final state
 *   (1.0f with loss 0), or 0x7fc00000 if the member is not in front there, which the definition rules out.  A w that is a
 *   NaN is stored as 0x7fc00000.  Entries at or beyond O stay untouched.
 *   - With loss 0 the nine shared outputs equal those of misift_adjust_bundle_batch byte for byte.  With loss 1 and
 *     every member's s <= c2 at every state visited (the states and the trial states) the same holds, and every member's
 *     weight is 1.0f.
 *   - An s that overflows to +inf: Huber gives w = 0 and rho = +inf, Geman-McClure gives w = 0 and a NaN rho; either way
 *     c is not finite and no step is kept.  Gate such observations out with max_error.
 *   - On the outlier scene of tests/test_filter_cpu.py one call with Huber at 2 px or Geman-McClure at 4 px brings the
 *     clean observations to the figures of tests/test_bundle_robust_cpu.py (MEASURED), where the plain call is held off
 *     by the outliers and adjust -> filter -> adjust removes clean observations with them.
 *   - Not done here: no robust loss in misift_refine_cameras_batch or misift_triangulate_tracks_batch, no Cauchy loss
 *     (its cost needs logf, which the arithmetic rules exclude), no second-order correction, the intrinsics are not
 *     refined (misift_adjust_bundle_focal_batch is this call with a focal scale per camera), the member set is not
 *     revised between steps (max_error is still the hard gate, decided once).
 *   - The argument errors of misift_adjust_bundle_batch; a loss other than 0, 1 or 2; with loss != 0 a loss_scale that
 *     is not finite and > 0: MISIFT_EINVAL, before anything is enqueued.  A d_obs_weight overlapping another buffer is
 *     the caller's error and is not checked.
 *   - Stream, copies and ordering as misift_adjust_bundle_batch.  The same memsets and launches, and one launch more
 *     with d_obs_weight (one lane per slot); the loss is uniform over the call, and loss 0 runs the kernels of the plain
 *     call.  The same temp memory: 100 bytes per slot, 76 per track and 352 per image, each array rounded up to 16. */
#define MISIFT_LOSS_NONE 0
#define MISIFT_LOSS_HUBER 1
#define MISIFT_LOSS_GEMAN_MCCLURE 2
int misift_adjust_bundle_robust_batch(misift_ctx *ctx,
                                      int max_tracks, int max_obs,
                                      const int *d_track_offsets,     /* max_tracks + 1, from export */
                                      const misift_track_obs *d_obs,  /* max_obs, from export, 16-byte aligned */
                                      const int *d_export_summary,    /* 8 ints, from export: [2] = T, [3] = O */
                                      const float *d_points,          /* max_tracks x 4, from triangulate */
                                      const int *d_point_status,      /* max_tracks, from triangulate */
                                      int nimages,
                                      const float *d_cam,             /* nimages x 12 */
                                      const int *d_cam_pair,          /* nimages */
                                      const float *intrinsics,        /* host, nimages x 4: fx fy cx cy, copied */
                                      int nhold, const int *hold,     /* host, images kept as they are, copied; may be NULL */
                                      int min_views, int min_obs, int num_loops, int cg_iters,
                                      float max_error, float lambda0, int orthonormalise,
                                      int loss, float loss_scale /* px */,
                                      float *d_cam_out,               /* nimages x 12; may be d_cam itself */
                                      float *d_points_out,            /* max_tracks x 4; may be d_points itself */
                                      int   *d_cam_obs,               /* nimages */
                                      int   *d_cam_status,            /* nimages */
                                      float *d_cam_rms,               /* nimages x 2: before, after */
                                      int   *d_point_obs,             /* max_tracks */
                                      float *d_history,               /* num_loops x 4 words */
                                      float *d_cost,                  /* 2: before, after */
                                      float *d_obs_weight,            /* max_obs; may be NULL */
                                      int   *d_summary);              /* 8 ints */

/* misift_adjust_bundle_robust_batch with one focal scale per physical camera among the unknowns (no reference
 * counterpart): every image is given the GROUP of the camera that took it, and each group g has one scalar s_g that
 * multiplies the given fx and fy of all its images.  A focal length from EXIF or guessed from the image width is
 * routinely 5 to 10 % off; this call estimates the correction jointly with the cameras and the points.  In the chain it
 * stands where adjust stands; a caller that carries on reads d_intrinsics_out back (16 * nimages bytes) and hands it
 * to the next call as its `intrinsics`.
 *   The arguments are those of misift_adjust_bundle_robust_batch in the same order, with `ngroups` and `group` after
 *   `loss_scale` and `d_intrinsics_out` and `d_focal` after `d_summary`.  ngroups lies in 0 ... MISIFT_MAX_FOCAL_GROUPS
 *   (8: a lane holds one 3-vector per group for its track, 24 registers, and forms them in one walk over the members; the
 *   constant also bounds the loops of the scalar workgroup and costs 32 bytes per track of temp).  group[i] is the group of image i, or -1 for an
 *   image whose intrinsics stay as given.  The definition is that of misift_adjust_bundle_robust_batch, every word of
 *   it, the arithmetic rules included, with the amendments below.  With ngroups == 0 or every group[i] == -1 there is no
 *   amendment: the call is the robust call.
 *   The unknown.  s_g = 1.0f at the start.  The sets are decided under the given intrinsics as there.  M_g = the
 *   members in the usable images of group g (an integer sum); a group with M_g == 0 is not LIVE: its s_g stays 1 and it
 *   takes no part below.  Wherever a member of an image i with g = group[i] >= 0 is projected under a state (the cost,
 *   step 1, d_obs_weight), the intrinsics are fx_i*s_g, fy_i*s_g, cx_i, cy_i with s_g of that state, each product
 *   rounded; an image with group -1 uses its four floats as given.
 *   Step 1.  Beside the 20 values a member of a grouped image has Juf = fx_i * a and Jvf = fy_i * b with the given fx_i,
 *   fy_i (and a, b of the view under the state); with loss != 0 both are multiplied by sw like the 20.  For such a
 *   member wf[q] = Juf*Pu[q] + Jvf*Pv[q], and wf . v = (wf[0]*v0 + wf[1]*v1) + wf[2]*v2 for a 3-vector v.
 *   Step 2.  Per active track and per live group g, after V' and y_t: w_gt = the per-track sum of wf over the track's
 *   members in images of group g (per component), and d_gt = (w_gt[0]*x0 + w_gt[1]*x1) + w_gt[2]*x2 with
 *   x = SOLVE(V', w_gt) (zeros when it fails).
 *   Step 3.  A usable image i with a group takes three more per-image sums, whatever its status: Uff_i with the term
 *   Juf*Juf + Jvf*Jvf, gf_i with Juf*ru + Jvf*rv, and wy_i with wf . y_t.  A free image with a group takes six more,
 *   Ucf_i[r] with Ju[r]*Juf + Jv[r]*Jvf: 42 sums in one pass.  U', b and M^-1 of a free image are unchanged.  Then per
 *   live group, in ascending g: U_gg, g_g and wy_g are the cross-image sums of Uff_i, gf_i and wy_i over the usable
 *   images of the group; D_g is the sum of d_gt over the active tracks by the 256-slot rule on the track index t (a
 *   track that is not active is skipped); UL_g = U_gg * l1, S_gg = UL_g - D_g, b_g = g_g - wy_g.  An S_gg that is not
 *   finite and > 0 makes the step FAIL like a failed SOLVE.
 *   Step 4.  PCG runs over the free images' 6-vectors and the live groups' scalars.  A dot product of two such vectors
 *   is the cross-image sum of the 6-vector dot products, to which v_g * w_g is added for each live group in ascending g,
 *   one at a time.  x_g = 0, r_g = b_g, z_g = r_g / S_gg, p_g = z_g.  In an iteration:
 *     the per-track sum for q_t takes, for each member in ascending slot, first (W^T p_i) if its image is free, then
 *     wf * p_g (per component) if its image has a group;
 *     a free image with a group has y_i[r] = (U'[r] . p_i + Ucf_i[r] * p_g) - (the per-image sum of (W q_t)[r]); and
 *     every usable image with a group takes the per-image sum wq_i of wf . q_t, a free one also c_i = Ucf_i . p_i (the
 *     6-vector dot product), any other c_i = 0;
 *     per live group y_g = (UL_g * p_g + the cross-image sum of c_i) - the cross-image sum of wq_i, both over the usable
 *     images of the group;
 *     sigma, alpha, rho', beta as there with the extended dot product; x_g += alpha*p_g, r_g -= alpha*y_g,
 *     z_g = r_g / S_gg, p_g = z_g + beta*p_g.
 *   Step 5.  The per-track sum of delta_t takes wf * x_g after (W^T x_i) in the same way.  The trial scale of a live
 *   group is s_g + x_g; one that is not finite and > 0 makes the trial state not finite (the step is turned away).
 *   Step 6 is unchanged: s_g is kept or turned away with the cameras and the points.
 *   Outputs.  The ten of misift_adjust_bundle_robust_batch.  d_intrinsics_out[4i..4i+3] = fx_i*s_g, fy_i*s_g (each
 *   rounded), cx_i, cy_i under the final state for a usable image of a group whose status is 0; the four input floats
 *   bit for bit for any other image.  d_focal[3g..3g+2] for g < ngroups: s_g of the final state (float), M_g (int),
 *   and the status (int): 0 MISIFT_FOCAL_REFINED, 1 MISIFT_FOCAL_NO_MEMBER (the group is not live), 2
 *   MISIFT_FOCAL_NOT_REFINED (num_loops == 0; s_g is 1.0f).  With every group[i] == -1, M_g is 0 and the status 1 (2
 *   with num_loops == 0).
 *   - With ngroups == 0, or every group[i] == -1, the ten shared outputs equal those of
 *     misift_adjust_bundle_robust_batch byte for byte (with loss 0 those of misift_adjust_bundle_batch too), the call
 *     launches that call's kernels, and d_intrinsics_out is the input bit for bit.  With num_loops == 0
 *     d_intrinsics_out is the input bit for bit and every s_g is 1.0f.
 *   - A held, root or demoted pose does not hold the focal scale: the members of such an image enter the focal sums.
 *     The gauge still needs two held poses (or a root and a held one); with fewer, scale and focal drift together.
 *   - The focal unknown is preconditioned by its own Schur scalar S_gg, not by its damped diagonal UL_g: with the plain
 *     diagonal PCG barely moves the focal scale (on 24 images, 400 tracks, 10 iterations it is still 7 % off after
 *     eight steps where S_gg leaves 0.5 %).
 *   - On planted scenes (120 tracks over 8 images and 400 over 24, 0.5 px noise) whose fx, fy are given 10 % off (one
 *     group), or 10 % short and long for two cameras taking turns, 8 steps at cg_iters 10 bring s_g within 1.34e-2
 *     (relative) of the planted 1 / 1.1 and 1 / 0.9 and within 1.27e-2 of a float64 Levenberg-Marquardt with every step
 *     solved exactly, and the pooled rms within 7.51e-3 px of that one's 0.46 px (MEASURED, the worst of the four scenes;
 *     tests/test_bundle_focal_cpu.py, which also holds fp32 to float64: 9.77e-4 on s_g, 1.73e-3 px on the rms).  The
 *     robust call on the same input ends at 0.58 to 10 px.
 *   - Not done here: no principal point, aspect ratio or distortion is estimated, there is no focal prior, and at most
 *     MISIFT_MAX_FOCAL_GROUPS groups; the other calls of the chain keep taking `intrinsics` from the host.
 *   - The argument errors of misift_adjust_bundle_robust_batch; ngroups outside 0 ... MISIFT_MAX_FOCAL_GROUPS; NULL
 *     group with ngroups > 0; a group[i] outside [-1, ngroups); NULL d_intrinsics_out; NULL d_focal with ngroups > 0:
 *     MISIFT_EINVAL, before anything is enqueued.  The new outputs overlapping another buffer is the caller's error.
 *   - Stream, copies and ordering as misift_adjust_bundle_batch; `group` is copied.  Without a grouped image: the
 *     memsets and launches of the robust call and one launch more (the two new outputs), the same temp.  With one: three
 *     memsets and 13 + num_loops * (8 + 3 * cg_iters) launches (one more with d_obs_weight): the groups' members in the
 *     scalar workgroup during the setup and the two new outputs at the end are the two more; the trial scale is set in
 *     the launch of the trial cameras and the groups' sums run in the scalar workgroup's existing launches.  The
 *     per-image pass of step 3 holds 42 sums (42 KiB of LDS).  Temp: 108 bytes per slot, 108 per track and 396 per
 *     image, each array rounded up to 16, and 320 bytes for the groups. */
#define MISIFT_MAX_FOCAL_GROUPS 8
#define MISIFT_FOCAL_REFINED 0
#define MISIFT_FOCAL_NO_MEMBER 1
#define MISIFT_FOCAL_NOT_REFINED 2
int misift_adjust_bundle_focal_batch(misift_ctx *ctx,
                                     int max_tracks, int max_obs,
                                     const int *d_track_offsets,     /* max_tracks + 1, from export */
                                     const misift_track_obs *d_obs,  /* max_obs, from export, 16-byte aligned */
                                     const int *d_export_summary,    /* 8 ints, from export: [2] = T, [3] = O */
                                     const float *d_points,          /* max_tracks x 4, from triangulate */
                                     const int *d_point_status,      /* max_tracks, from triangulate */
                                     int nimages,
                                     const float *d_cam,             /* nimages x 12 */
                                     const int *d_cam_pair,          /* nimages */
                                     const float *intrinsics,        /* host, nimages x 4: fx fy cx cy, copied */
                                     int nhold, const int *hold,     /* host, images kept as they are, copied; may be NULL */
                                     int min_views, int min_obs, int num_loops, int cg_iters,
                                     float max_error, float lambda0, int orthonormalise,
                                     int loss, float loss_scale /* px */,
                                     int ngroups, const int *group,  /* host, nimages: the group of the image or -1, copied */
                                     float *d_cam_out,               /* nimages x 12; may be d_cam itself */
                                     float *d_points_out,            /* max_tracks x 4; may be d_points itself */
                                     int   *d_cam_obs,               /* nimages */
                                     int   *d_cam_status,            /* nimages */
                                     float *d_cam_rms,               /* nimages x 2: before, after */
                                     int   *d_point_obs,             /* max_tracks */
                                     float *d_history,               /* num_loops x 4 words */
                                     float *d_cost,                  /* 2: before, after */
                                     float *d_obs_weight,            /* max_obs; may be NULL */
                                     int   *d_summary,               /* 8 ints */
                                     float *d_intrinsics_out,        /* nimages x 4 */
                                     int   *d_focal);                /* ngroups x 3 words: s_g, M_g, status */

/* THE RADIAL MODEL of misift_adjust_bundle_radial_batch and misift_undistort_obs_batch: one coefficient k_g per camera
 * group, applied to the OBSERVATION, not to the projection (so the 20 values of step 1 are what they were and
 * undistorting is closed-form).  For an observation (x, y) of image i with the GIVEN fx, fy, cx, cy, g = group[i] >= 0
 * and k = k_g:
 *     dx = x - cx;  dy = y - cy;  nx = dx / fx;  ny = dy / fy;
 *     rho2 = nx*nx + ny*ny;  e = k * rho2;
 *     x' = x + dx*e;  y' = y + dy*e;
 * every operation fp32 and rounded on its own, no contraction.  With k == 0 and a finite rho2, x' == x and y' == y (a
 * zero of either sign is added).  An observation so far out that rho2 overflows (beyond about 1.8e19 focal lengths
 * from the principal point) gives NaN whatever k is; nearer ones can still overflow dx*rho2 or dx*e (1e20 px at a focal
 * length of 500 does) and give an infinite or NaN x' unless k == 0.  rho2 always
 * takes the given fx, fy, never the scaled ones of the focal call: k_g is a coefficient relative to the given
 * intrinsics and its derivative column does not depend on the state.  An image with group[i] == -1 uses x, y as given.
 *
 * misift_adjust_bundle_focal_batch with k_g among the unknowns (no reference counterpart).  A few percent of radial
 * displacement at the image corners is tens of pixels at 1920 x 1080: the hard gates throw such observations away and a
 * robust loss bends the solution to the image centre.  In the chain it stands where adjust stands, and
 * misift_undistort_obs_batch behind it hands every later call an undistorted list, so that they stay pinhole.
 *   The arguments are those of misift_adjust_bundle_focal_batch in the same order, with `radial` and `k0` after `group`
 *   and `d_radial` after `d_focal`.  radial[g] is 1 when k_g is an unknown and 0 when it is held at k0[g]; k0[g] is the
 *   value every state starts with.  Both NULL means all zero; one NULL without the other is an error.  ngroups lies in
 *   0 ... MISIFT_MAX_RADIAL_GROUPS, which is MISIFT_MAX_FOCAL_GROUPS: the per-track 3-vectors of the coefficients are
 *   formed in a walk of their own over the members, in the registers the focal ones have left, so the count of groups
 *   did not have to come down (no scratch memory in any instance).
 *   The definition is that of misift_adjust_bundle_focal_batch, every word of it, with the amendments below.
 *   Observations.  Wherever an observation of a grouped image enters, it is (x', y') under k_g of that state: in the
 *   member test (under the start state, k_g = k0[g]), in the cost, in step 1 and in d_obs_weight.
 *   The unknown.  k_g = k0[g] at the start.  A group is RADIAL-LIVE when radial[g] == 1 and it is live (M_g > 0).
 *   Step 1.  A member of a group with radial[g] == 1 has one more column: Juk = -(dx*rho2), Jvk = -(dy*rho2), each
 *   product rounded and then negated.  The sign: ru = x' - u grows by dx*rho2 per unit of k, and every column J of the
 *   definition is such that r falls by J times the step, so the column is the negative of that growth.  Under a loss
 *   both are multiplied by sw like the 20.  For such a member wk[q] = Juk*Pu[q] + Jvk*Pv[q].
 *   Step 2.  Per active track and per radial-live group, after the d_gt: wk_gt = the per-track sum of wk over the
 *   track's members in images of group g, and dk_gt = wk_gt . SOLVE(V', wk_gt) as d_gt.
 *   Step 3.  A usable image of a group with radial[g] == 1 takes four more per-image sums, whatever its status: Ukk_i
 *   (Juk*Juk + Jvk*Jvk), gk_i (Juk*ru + Jvk*rv), wyk_i (wk . y_t) and Ufk_i (Juf*Juk + Jvf*Jvk); a free one six more,
 *   Uck_i[r] = Ju[r]*Juk + Jv[r]*Jvk: 52 sums in one pass, in the order the 33, Ucf, the focal three, Uck, these four.
 *   Per radial-live group in ascending g, after all the focal scalars: U_kk, g_k, wy_k and U_fk are the cross-image sums
 *   over the usable images of the group, Dk_g the sum of dk_gt by the 256-slot rule on t; UL_k = U_kk * l1,
 *   S_kk = UL_k - Dk_g, b_k = g_k - wy_k.  An S_kk that is not finite and > 0 makes the step FAIL.  U_fk is not damped.
 *   Step 4.  The PCG vector gains one scalar per radial-live group, appended after the focal scalars in ascending g: a
 *   dot product adds v_k * w_k for each, one at a time, after the focal ones.  x_k = 0, r_k = b_k, z_k = r_k / S_kk,
 *   p_k = z_k.  In an iteration:
 *     the per-track sum takes, for each member, after wf * p_g, wk * p_k (per component) if radial[g] == 1;
 *     a free image of such a group has y_i[r] = ((U'[r] . p_i + Ucf_i[r]*p_g) + Uck_i[r]*p_k) - (the sum of (W q_t)[r]);
 *     every usable image of such a group takes the per-image sum wqk_i of wk . q_t, a free one also ck_i = Uck_i . p_i;
 *     per radial-live group y_g = ((UL_g*p_g + U_fk*p_k) + the sum of c_i) - the sum of wq_i, and
 *     y_k = ((UL_k*p_k + U_fk*p_g) + the cross-image sum of ck_i) - the cross-image sum of wqk_i;
 *     x_k += alpha*p_k, r_k -= alpha*y_k, z_k = r_k / S_kk, p_k = z_k + beta*p_k.
 *   Step 5.  The per-track sum of delta_t takes wk * x_k in the same way.  The trial coefficient of a radial-live group
 *   is k_g + x_k; one that is not finite makes the trial state not finite.  Any other k_g stays.
 *   Step 6.  s_g, k_g, the cameras and the points are kept or turned away together.
 *   Outputs.  The ten shared ones; d_intrinsics_out and d_focal exactly as in the focal call; d_radial[3g..3g+2] for
 *   g < ngroups: k_g of the final state (float), M_g (int, the word of d_focal), and the status (int):
 *   3 MISIFT_RADIAL_HELD when radial[g] == 0 (k_g is k0[g]), otherwise 2 MISIFT_RADIAL_NOT_REFINED with
 *   num_loops == 0, otherwise 0 MISIFT_RADIAL_REFINED for a radial-live group and 1 MISIFT_RADIAL_NO_MEMBER for any other.
 *   - Identity.  With ngroups == 0, or every group[i] == -1, or every radial[g] == 0 and every k0[g] == 0, the call
 *     launches the kernels of misift_adjust_bundle_focal_batch and one launch more (d_radial, with ngroups > 0), with that
 *     call's temp; the twelve shared outputs are that call's byte for byte.
 *   - The two scalars of a group are preconditioned each by its own Schur scalar (S_gg, S_kk), not by their 2 x 2 Schur
 *     block [[S_gg, S_fk], [S_fk, S_kk]].  MEASURED in float64 restatements on the four recovery scenes below, 8 steps at
 *     cg_iters 10, against a Levenberg-Marquardt with every step solved exactly, worst case: the two diagonals end
 *     within 1.27e-2 (k_g, in units of the planted coefficient) and 1.26e-2 (s_g, relative) of it, the 2 x 2 block
 *     within 2.84e-2 and 1.79e-2.  The block is not closer, so the simpler choice stands and S_fk is not formed.
 *   - On planted scenes (120 tracks over 8 images and 400 over 24, 0.5 px noise) displaced by the model itself with
 *     k = -0.15 (one group), or -0.15 and +0.08 for two cameras taking turns, at the normalised corner radius of the
 *     image, the focal given 10 % off, 8 steps at cg_iters 10 bring k_g within 7.46e-2 of the planted coefficient (in
 *     units of it; 1.65e-2 with one group) and s_g within 1.42e-2, and the pooled rms within 7.99e-3 px of the exact
 *     Levenberg-Marquardt's 0.46 px (MEASURED, the worst of the four scenes; tests/test_bundle_radial_cpu.py, which
 *     also holds fp32 to float64: 3.12e-2 on k_g, 1.02e-3 on s_g, 1.20e-3 px on the rms).  The focal call on the same
 *     input ends at 1.30 to 2.09 px.  A scene planted with the forward model x_d = x_u*(1 + k*r_u^2) instead (120 tracks,
 *     8 images, one group) is left at 0.484 px by this one-parameter inverse model where the focal call leaves 1.09 px.
 *   - Not done here: one coefficient only (no k2, no tangential terms, no principal point); no prior on k; no check
 *     that 1 + 3*k*rho2 stays positive over the image (where it does not, the model folds over).  The model is the
 *     inverse (undistorting) one: a k from a forward-model calibration x_d = x_u*(1 + k*r_u^2) has roughly the opposite
 *     sign.
 *   - The argument errors of misift_adjust_bundle_focal_batch; a radial[g] that is not 0 or 1; a k0[g] that is not
 *     finite; one of radial and k0 NULL without the other; NULL d_radial with ngroups > 0: MISIFT_EINVAL, before anything
 *     is enqueued.
 *   - Stream, copies and ordering as misift_adjust_bundle_focal_batch; `radial` and `k0` are copied.  With a grouped image
 *     and a radial[g] == 1 or a k0[g] != 0: three memsets and 14 + num_loops * (8 + 3 * cg_iters) launches (one more with
 *     d_obs_weight), launch for launch the focal call's with the d_radial launch at the end.  The column Juk, Jvk is
 *     stored per slot once per step (8 bytes) beside Juf, Jvf: a per-track pass then reads 8 bytes where recomputing
 *     would read the 16-byte observation, the image's 16 bytes and sw.  The per-image pass of step 3 holds 52 sums
 *     (52 KiB of LDS).  Temp: 116 bytes per slot, 140 per track and 444 per image, each array rounded up to 16, and 640
 *     bytes for the groups. */
#define MISIFT_MAX_RADIAL_GROUPS MISIFT_MAX_FOCAL_GROUPS
#define MISIFT_RADIAL_REFINED 0
#define MISIFT_RADIAL_NO_MEMBER 1
#define MISIFT_RADIAL_NOT_REFINED 2
#define MISIFT_RADIAL_HELD 3
int misift_adjust_bundle_radial_batch(misift_ctx *ctx,
                                      int max_tracks, int max_obs,
                                      const int *d_track_offsets,     /* max_tracks + 1, from export */
                                      const misift_track_obs *d_obs,  /* max_obs, from export, 16-byte aligned */
                                      const int *d_export_summary,    /* 8 ints, from export: [2] = T, [3] = O */
                                      const float *d_points,          /* max_tracks x 4, from triangulate */
                                      const int *d_point_status,      /* max_tracks, from triangulate */
                                      int nimages,
                                      const float *d_cam,             /* nimages x 12 */
                                      const int *d_cam_pair,          /* nimages */
                                      const float *intrinsics,        /* host, nimages x 4: fx fy cx cy, copied */
                                      int nhold, const int *hold,     /* host, images kept as they are, copied; may be NULL */
                                      int min_views, int min_obs, int num_loops, int cg_iters,
                                      float max_error, float lambda0, int orthonormalise,
                                      int loss, float loss_scale /* px */,
                                      int ngroups, const int *group,  /* host, nimages: the group of the image or -1, copied */
                                      const int *radial,              /* host, ngroups: 1 = k_g is an unknown, copied; may be NULL */
                                      const float *k0,                /* host, ngroups: k_g at the start, copied; NULL with radial */
                                      float *d_cam_out,               /* nimages x 12; may be d_cam itself */
                                      float *d_points_out,            /* max_tracks x 4; may be d_points itself */
                                      int   *d_cam_obs,               /* nimages */
                                      int   *d_cam_status,            /* nimages */
                                      float *d_cam_rms,               /* nimages x 2: before, after */
                                      int   *d_point_obs,             /* max_tracks */
                                      float *d_history,               /* num_loops x 4 words */
                                      float *d_cost,                  /* 2: before, after */
                                      float *d_obs_weight,            /* max_obs; may be NULL */
                                      int   *d_summary,               /* 8 ints */
                                      float *d_intrinsics_out,        /* nimages x 4 */
                                      int   *d_focal,                 /* ngroups x 3 words: s_g, M_g, status */
                                      float *d_radial);               /* ngroups x 3 words: k_g, M_g, status */

/* An observation list undistorted under THE RADIAL MODEL above with the coefficients misift_adjust_bundle_radial_batch
 * left on the device (no reference counterpart): ... -> refine -> adjust_bundle_radial -> undistort_obs -> triangulate /
 * filter / adjust / resect on the undistorted list with d_intrinsics_out, all of them pinhole and unchanged.
 *   For every slot o < min(max(O, 0), max_obs), with O read on the device from d_export_summary[3]: frame and record
 *   are copied; xpos, ypos become x', y' under k = d_radial[3g] (whatever the group's status) when the frame lies in
 *   [0, nimages) and g = group[frame] >= 0, otherwise they are copied bit for bit.  Slots from O on are untouched.
 *   `intrinsics` are the GIVEN ones, those the radial call was given.  ngroups == 0: every slot is copied.
 *   - d_obs_out may be d_obs itself; any other overlap, a d_obs or d_obs_out that is not 16-byte aligned, NULL d_obs,
 *     d_export_summary, intrinsics or d_obs_out, NULL group or d_radial with ngroups > 0, max_obs or nimages < 1,
 *     ngroups outside 0 ... MISIFT_MAX_RADIAL_GROUPS, a group[i] outside [-1, ngroups), unusable intrinsics:
 *     MISIFT_EINVAL, before anything is enqueued.
 *   - One launch on the context stream, one lane per slot, one 16-byte load and one 16-byte store; no temp memory, no
 *     host read; `intrinsics` and `group` are copied. */
int misift_undistort_obs_batch(misift_ctx *ctx,
                               int max_obs,
                               const misift_track_obs *d_obs,         /* max_obs, 16-byte aligned */
                               const int *d_export_summary,           /* 8 ints, from export: [3] = O */
                               int nimages,
                               const float *intrinsics,               /* host, nimages x 4, the given ones, copied */
                               int ngroups, const int *group,         /* host, nimages, copied */
                               const float *d_radial,                 /* ngroups x 3 words, from the radial call */
                               misift_track_obs *d_obs_out);          /* max_obs; may be d_obs itself */

/* The observation lists of misift_export_tracks_batch gated against the current points and cameras and written out
 * again, compact and in export's own format (no reference counterpart): per observation the reprojection error, per
 * track the duplicate frames, the number of views and the triangulation angle.  It is what "gate on d_obs_error and call
 * again" (triangulate), "a hard gate, decided once" (refine) and "the member set is not revised between steps" (adjust)
 * leave to the caller, done on the device: adjust -> filter -> triangulate or adjust on the filter's outputs, with no
 * list read back.  Every later call (triangulate, refine, resect, adjust) takes the outputs unchanged.
 *   The inputs are those of misift_refine_cameras_batch and are read as there: d_track_offsets, d_obs and
 *   d_export_summary from export (or from an earlier call of this one), d_points and d_point_status from triangulate or
 *   adjust, d_cam and d_cam_pair, intrinsics[4i..4i+3] = fx fy cx cy.  obs.record and d_points[4t+3] are not read.
 *   The arithmetic is that of misift_refine_cameras_batch: fp32, every operation rounded, only + - * / and sqrtf, no
 *   contraction, a comparison with a NaN is false, everything left to right as written; a . b = (a0*b0 + a1*b1) + a2*b2.
 *   T, O, VALID tracks and the OWNER of a slot are those of misift_refine_cameras_batch.
 *   1. Per slot o < O, the first reason that applies:
 *        -1  the slot has no owner;
 *        -2  its owner t has d_point_status[t] != 0 or a non-finite X = d_points[4t..4t+2];
 *        -3  the view is not USABLE in the sense of step 1 of misift_triangulate_tracks_batch: its frame f outside
 *            [0, nimages), d_cam_pair[f] == -2, a non-finite float among d_cam[12f..], or a non-finite x or y;
 *        -4  Xc.z > 0 is false;
 *        -5  e2 < E2 is false, with e2 = ru*ru + rv*rv exactly as in step 2 of misift_refine_cameras_batch and
 *            E2 = max_error*max_error rounded once on the host.  The test is plain: there is no special case for +inf,
 *            so a NaN or +inf e2 never passes.
 *      A slot with none of these reasons is a SURVIVOR with its e2.
 *   2. Duplicates, with unique_frames == 1.  Survivor o LOSES (-6) iff another survivor o' of the same track and frame has
 *      e2' < e2, or e2' == e2 and o' < o.  The KEPT views of track t are its survivors that did not lose (all of them
 *      with unique_frames == 0); m = their number.
 *   3. Per track t < T: d_track_map[t] = -1 if the track is not valid; -2 if its point is bad as in rule 1; -7 if
 *      m < min_views; -8 if max_cos < +inf and NO pair k < l of its kept views has u_k . u_l < max_cos.  Per kept view,
 *      with r0, r1, r2 the rows of R_f: C[c] = -((r0[c]*t0 + r1[c]*t1) + r2[c]*t2), d = X - C per component,
 *      n = sqrtf(d . d), u = d / n per component: the unit ray from the camera centre to the point.  max_cos is the
 *      cosine of the smallest triangulation angle the caller accepts, passed as a float so that no cosf stands between
 *      this text and its restatement; +inf switches the test off.  "A pair exists" does not depend on an order, so the
 *      decision is pinned without pinning a reduction order.  A point on a camera centre gives n = 0 and a NaN ray,
 *      which is wide apart from nothing.  The kept views of a track dropped with -7 or -8 get that code in d_obs_map;
 *      every other slot keeps its own reason.
 *   4. Numbering.  The surviving tracks are numbered t' = 0, 1, ... in ascending t; off'[t'] = the sum of m over the
 *      surviving tracks before it; within a track the kept views go in ascending slot.  d_obs_out[off' + k] = the 16
 *      input bytes of the k-th kept view, bit for bit; d_track_offsets_out[0 .. T'] = off' ([0] = 0 always);
 *      d_points_out[4t' .. 4t'+2] = the three input words, bit for bit; d_points_out[4t'+3] = sqrtf(s / (float)m), s the
 *      sum of the kept e2 in ascending slot, from +0, one term at a time; d_point_views_out[t'] = m;
 *      d_point_status_out[t'] = 0; d_track_map[t] = t'; d_obs_map[o] = the new slot.  Entries at or beyond T' (beyond
 *      T' + 1 of the offsets) and O', beyond T of d_track_map and beyond O of d_obs_map stay untouched.
 *   5. d_export_summary_out (8 ints) has export's layout; the result is never larger than the input, so nothing is cut:
 *      [0] = [2] = T', [1] = [3] = O', [4] = the largest m kept (0 if none), [5] = [6] = [7] = 0.
 *   6. d_summary (8 ints, integer sums): [0] T', [1] O', [2] slots with -4, [3] with -5, [4] with -6, [5] tracks with
 *      -7, [6] tracks with -8, [7] slots with -1, -2 or -3.
 *   - Deterministic: byte-identical from run to run.  Every index read from device memory (T, O, offsets, frames) is
 *     range-checked before it addresses anything.
 *   - Idempotent: run on its own outputs with the same arguments it keeps everything: T'' = T', O'' = O', the same bytes.
 *   - With max_error = +inf, max_cos = +inf, unique_frames = 0 and min_views = 2 on export's and triangulate's own output
 *     it drops exactly the tracks triangulate did not give status 0, and the views triangulate did not use or that lie
 *     behind a camera.
 *   - Not done here: no robust re-weighting (the gate is hard: misift_adjust_bundle_robust_batch weighs the observations
 *     down instead of removing them); the records it removes are not merged into new tracks;
 *     the points are not re-estimated (d_points_out[4t'+3] is the rms of the kept views under the OLD point), so call
 *     triangulate or adjust afterwards.
 *   - NULL ctx; max_tracks, max_obs or nimages < 1; a NULL pointer other than d_obs_map; d_obs or d_obs_out not 16-byte
 *     aligned; min_views < 2; unique_frames other than 0 or 1; max_error NaN or <= 0; max_cos NaN; an fx or fy that is
 *     not finite and > 0 or a cx or cy that is not finite; an output overlapping an input or another output, each taken
 *     at its stated size (in place is NOT supported: compaction moves entries across workgroups): MISIFT_EINVAL, before
 *     anything is enqueued.  None of the inputs is written.
 *   - The call runs on the context stream and returns before the GPU work is done; `intrinsics` is copied; no host
 *     synchronisation and no host read.  Ordering behind batches in flight (K > 1): as misift_match_batch.
 *   - One copy, three memsets and six launches whatever the data: the owners, one lane per slot for rule 1, one wavefront
 *     per track for rules 2 and 3 (its first 256 views staged on chip, a longer track reads the rest from temp memory),
 *     the scan of 2048-track tile sums in one workgroup, one lane per track for the numbering, one wavefront per track
 *     for the copy; no workgroup waits for another.  Temp memory from the library's own allocator, sized from the
 *     capacities only: 24 bytes per slot, 8 per track plus 8 per 2048 tracks, and 16 per image, each array rounded up
 *     to 16. */
int misift_filter_tracks_batch(misift_ctx *ctx,
                               int max_tracks, int max_obs,
                               const int *d_track_offsets,     /* max_tracks + 1, from export */
                               const misift_track_obs *d_obs,  /* max_obs, from export, 16-byte aligned */
                               const int *d_export_summary,    /* 8 ints, from export: [2] = T, [3] = O */
                               const float *d_points,          /* max_tracks x 4, from triangulate or adjust */
                               const int *d_point_status,      /* max_tracks, from triangulate */
                               int nimages,
                               const float *d_cam,             /* nimages x 12 */
                               const int *d_cam_pair,          /* nimages */
                               const float *intrinsics,        /* host, nimages x 4: fx fy cx cy, copied */
                               float max_error, float max_cos, int min_views, int unique_frames,
                               int *d_track_offsets_out,       /* max_tracks + 1 */
                               misift_track_obs *d_obs_out,    /* max_obs, 16-byte aligned */
                               int *d_export_summary_out,      /* 8 ints, export's layout */
                               float *d_points_out,            /* max_tracks x 4 */
                               int *d_point_views_out,         /* max_tracks */
                               int *d_point_status_out,        /* max_tracks */
                               int *d_track_map,               /* max_tracks: t' or the reason */
                               int *d_obs_map,                 /* max_obs: the new slot or the reason; may be NULL */
                               int *d_summary);                /* 8 ints */

/* cudaMallocManaged as used by the reference's MANAGEDMEM build flavour (cudaSiftH.cu:239-240): one pointer valid on
 * host and device (SiftData.m_data). */
int misift_malloc_managed(size_t bytes, void **out);

/* Test-only entry point (no reference counterpart): the device copies of the written-out elementary functions that
 * replace CUDA's exp2f / atan2f / expf / __sinf,__cosf (cudaSiftD.cu:1417, 1008, 987, 331-332), evaluated on n inputs.
 * fn: 0 = exp2(x), 1 = atan2(y, x), 2 = exp(x), 3 = sin/cos(x) -> d_out, d_out2.  Device pointers; synchronous. */
int misift_test_elementary(misift_ctx *ctx, int fn, const float *d_x, const float *d_y, float *d_out, float *d_out2,
                           int n);

/* Test-only: MatchSiftData with the column sweep cut the way misift_match_sharded cuts it (64-column super-tiles
 * [own_tile_begin, own_tile_end) in a first launch, all others in a second, one merge).  Same results as misift_match. */
int misift_test_match_split(misift_ctx *ctx, void *d_pts1, int n1, const void *d_pts2, int n2, int own_tile_begin,
                            int own_tile_end);

/* Test-only, host-only (no device needed): the matcher's column-chunk plan for n1 x n2 on a chip of num_cus CUs. */
int misift_test_match_plan(int num_cus, int n1, int n2, int *nchunks, int *tiles_per_chunk, int *ntiles);
/* Test-only, host-only: the work list misift_match_batch's plan kernel builds for pairs of n1[i] x n2[i] records on a chip
 * of num_cus CUs, in the context's match_full mode.  plan5[5i..5i+4] = first work item, 128-row blocks, 64-column
 * super-tiles, column chunks, super-tiles per chunk of pair i (items of a pair: row block major, chunk minor);
 * *nitems = items in all; *chunks = the call's chunk count (1: no column split, no partials); *partial_items_bound =
 * the items the partials buffer holds, which a call with *chunks > 1 never exceeds. */
int misift_test_match_batch_plan(int num_cus, int match_full, int npairs, const int *n1, const int *n2, int *plan5,
                                 int *nitems, int *chunks, int *partial_items_bound);
/* Test-only, host-only: the libc rand() misift_find_homography_batch restates on the device: out[k] = the k-th rand()
 * after srand(seed), k < n.  And the sample positions it draws: out[4 * loop + j] = position j (in the ordered list of
 * num_valid >= 8 valid points) of hypothesis loop, in the reference's rejection-loop order (matching.cu:1041-1053). */
int misift_test_libc_rand(unsigned seed, int n, int *out);
int misift_test_homography_samples(unsigned seed, int num_valid, int num_loops, int *out);
/* Test-only, host-only: what misift_find_fundamental_batch / misift_score_fundamental_batch run on the device, compiled
 * from the same headers.  The sample positions: out[8 * loop + j] = position j (in the ordered list of num_valid >= 8
 * valid records) of hypothesis loop after srand(seed).  The 8-point solve of one sample xy[4k..4k+3] = x1 y1 x2 y2 of
 * match k < 8: F9 (nine zeros when invalid) and *valid = 0 / 1.  And the Sampson terms of n matches under F9:
 * e2_out[i] = e*e, den_out[i] = den.  And match_error as score stores it: out[i] from e2[i] and den[i]. */
int misift_test_fundamental_samples(unsigned seed, int num_valid, int num_loops, int *out);
int misift_test_fundamental_solve(const float *xy, float *F9, int *valid);
int misift_test_fundamental_sampson(const float *F9, const float *xy, int n, float *e2_out, float *den_out);
int misift_test_fundamental_error(const float *e2, const float *den, int n, float *out);
/* Test-only, host-only: the rounds of misift_improve_fundamental_batch on plain arrays, compiled from the function the
 * kernel runs (the 256 slots of the call's sum one after another).  xy[4r..4r+3] = x1 y1 x2 y2 of record r < n, gate[r]
 * != 0 iff it passes the gate; F9_in the start; F9_out, *num_fit and *num_rounds as the call returns them.  And the
 * records of a frame the kernel stages on chip; a frame may hold more. */
int misift_test_fundamental_refine(const float *xy, const unsigned char *gate, int n, const float *F9_in, float thresh,
                                   int num_loops, float *F9_out, int *num_fit, int *num_rounds);
int misift_test_fundamental_refine_capacity(void);
/* Test-only, host-only: the eight elimination steps, the back-substitution and the permutation undone on the 9x9 matrix
 * M81 (row-major): n9 = Fn, *valid = whether every pivot was non-zero and finite.  lanes = 0: the serial form, the
 * template of the 8-point solve at nine rows; lanes = 1: the form the kernel spreads over 81 threads and the hook above
 * runs, its lanes one after another.  Equal bits. */
int misift_test_fundamental_solve9(const float *M81, int lanes, float *n9, int *valid);
/* Test-only, host-only: steps 1-4 and steps 5 and 7 of misift_recover_pose_batch, compiled from the functions the kernel
 * runs.  decompose: out48[12k..12k+11] = R and t of hypothesis k of F9 under K8 (fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2), and
 * *valid = 1; an invalid entry gives 48 zeros and 0.  vote: for record r < n with xy[4r..4r+3] = x1 y1 x2 y2, under
 * pose12 = R then t: front_out[r] = 1 iff it is in front, xyz_out[4r..4r+3] = what d_xyz gets. */
int misift_test_pose_decompose(const float *F9, const float *K8, float *out48, int *valid);
int misift_test_pose_vote(const float *pose12, const float *K8, const float *xy, int n, unsigned char *front_out,
                          float *xyz_out);
/* Test-only, host-only: steps 3-6 with the two F of step 7, and steps 1 and 7 record by record, of
 * misift_recover_pose_planar_batch, compiled from the functions the kernel runs.  decompose: *model = -1, 1 or 2 for H9
 * under K8 and min_baseline; out84 = s1, s3, then for k = 0..3 R and t (12) and N and d (4) of hypothesis k, then F_0 and
 * F_2 (9 each).  Model 2 gives R, t = 0 and zeros for the planes and the F; model -1 gives 84 zeros.  vote: for record
 * r < n with xy[4r..4r+3] = x1 y1 x2 y2 and gate[r] = whether it passes the gate: h_in[r] = 1 iff it is an H-inlier of H9
 * at thresh_h, f_in[r] = 1 iff F9 is given and it is an inlier of F9 at thresh_f, votes[4r+k] = 1 iff it counts for
 * hypothesis k of hyp84 (decompose's out84) at thresh_f; decision9 = nH, nF, 1 iff step 2 lets the entry go on under
 * planar_ratio and min_inliers (F9 NULL: no F is given), the four votes, the pick and the alternative of step 7.  The d_xyz
 * rows are those of misift_test_pose_vote. */
int misift_test_pose_planar_decompose(const float *H9, const float *K8, float min_baseline, float *out84, int *model);
int misift_test_pose_planar_vote(const float *H9, const float *F9, const float *hyp84, const float *K8, const float *xy,
                                 const unsigned char *gate, int n, float thresh_h, float thresh_f, float planar_ratio,
                                 int min_inliers, unsigned char *h_in, unsigned char *f_in, unsigned char *votes,
                                 int *decision9);
/* Test-only, host-only: step 1 of misift_link_poses_batch for one link and steps 2 and 3 for a whole graph, compiled from
 * the functions the kernels run.  ratio: rows_p / rows_q are row 0 of the two pairs (host memory, 576-byte records),
 * xyz_p / xyz_q their d_xyz rows, count_p / count_q their row counts as d_row_counts holds them; *ratio and *common = what
 * d_link_ratio and d_link_common get (the median taken from a sorted copy).  compose: everything on the host, ratio = the
 * links' d_link_ratio; pair_scale, cam and cam_pair as the call writes them, counts2 = summary [1] and [2].  capacity:
 * which = 0: the rows of a link whose rho bits the ratio kernel stages on chip; which = 1: the words of lists and state
 * (4 per link, 4 per pair, 1 per walk entry, 13 per image) up to which the second kernel works on chip. */
int misift_test_posegraph_ratio(const void *rows_p, const float *xyz_p, int count_p, const void *rows_q,
                                const float *xyz_q, int count_q, int max_pts, int kind, float min_score,
                                float max_ambiguity, float max_error, int min_common, float *ratio, int *common);
int misift_test_posegraph_compose(int npairs, const int *pairs, int nimages, const float *pose, const int *num_front,
                                  int nlinks, const int *links, const float *ratio, int seed_pair, int root_image,
                                  int nwalk, const int *walk, float *pair_scale, float *cam, int *cam_pair, int *counts2);
int misift_test_posegraph_capacity(int which);
/* Test-only, host-only: steps 1-5 of misift_triangulate_tracks_batch for one track, compiled from the function a lane of
 * the kernel runs.  cams (nimages x 12), cam_pair (nimages) and intrinsics (nimages x 4) on the host, obs the track's nobs
 * observations; point4, *views, *status and obs_error (nobs floats, may be NULL) as the call writes them for a track
 * whose range is valid, *gn_accepted = the Gauss-Newton steps kept.  capacity: the images whose cameras and intrinsics
 * the kernel holds on chip; a call may have more. */
int misift_test_triangulate_track(const float *cams, const int *cam_pair, const float *intrinsics, int nimages,
                                  const misift_track_obs *obs, int nobs, int min_views, int num_loops, float *point4,
                                  int *views, int *status, float *obs_error, int *gn_accepted);
int misift_test_triangulate_capacity(void);
/* Test-only, host-only: steps 0-7 of misift_refine_cameras_batch for one image, compiled from the function its workgroup
 * runs, the 256 slots of the sum one after another.  cam12 its camera, cam_pair its d_cam_pair entry, held != 0 iff it is
 * in `hold`, intrinsics4 its fx fy cx cy; its ncand candidates as slot[] (their slot indices o, >= 0 and ascending),
 * X[3k..3k+2] and xy[2k..2k+1].  cam_out12 (may be cam12), *nobs, rms2[0..1], *steps and *status as the call writes them. */
int misift_test_refine_camera(const float *cam12, int cam_pair, int held, const float *intrinsics4, int ncand,
                              const int *slot, const float *X, const float *xy, int min_obs, int num_loops,
                              float max_error, int orthonormalise, float *cam_out12, int *nobs, float *rms2, int *steps,
                              int *status);
/* Test-only, host-only: the whole of misift_adjust_bundle_batch on host arrays, every phase compiled from the function
 * its kernel runs (bundle_core.hpp).  The arguments are those of the call without the context; all pointers are host. */
int misift_test_adjust_bundle(int max_tracks, int max_obs, const int *track_offsets, const misift_track_obs *obs,
                              const int *export_summary, const float *points, const int *point_status, int nimages,
                              const float *cam, const int *cam_pair, const float *intrinsics, int nhold, const int *hold,
                              int min_views, int min_obs, int num_loops, int cg_iters, float max_error, float lambda0,
                              int orthonormalise, float *cam_out, float *points_out, int *cam_obs, int *cam_status,
                              float *cam_rms, int *point_obs, float *history, float *cost, int *summary);
/* The same for misift_adjust_bundle_robust_batch; misift_test_adjust_bundle is this one with loss 0 and no obs_weight. */
int misift_test_adjust_bundle_robust(int max_tracks, int max_obs, const int *track_offsets, const misift_track_obs *obs,
                                     const int *export_summary, const float *points, const int *point_status,
                                     int nimages, const float *cam, const int *cam_pair, const float *intrinsics,
                                     int nhold, const int *hold, int min_views, int min_obs, int num_loops, int cg_iters,
                                     float max_error, float lambda0, int orthonormalise, int loss, float loss_scale,
                                     float *cam_out, float *points_out, int *cam_obs, int *cam_status, float *cam_rms,
                                     int *point_obs, float *history, float *cost, float *obs_weight, int *summary);
/* The same for misift_adjust_bundle_focal_batch; misift_test_adjust_bundle_robust is this one with ngroups 0 and neither
 * intrinsics_out nor focal. */
int misift_test_adjust_bundle_focal(int max_tracks, int max_obs, const int *track_offsets, const misift_track_obs *obs,
                                    const int *export_summary, const float *points, const int *point_status,
                                    int nimages, const float *cam, const int *cam_pair, const float *intrinsics,
                                    int nhold, const int *hold, int min_views, int min_obs, int num_loops, int cg_iters,
                                    float max_error, float lambda0, int orthonormalise, int loss, float loss_scale,
                                    int ngroups, const int *group, float *cam_out, float *points_out, int *cam_obs,
                                    int *cam_status, float *cam_rms, int *point_obs, float *history, float *cost,
                                    float *obs_weight, int *summary, float *intrinsics_out, int *focal);
/* The same for misift_adjust_bundle_radial_batch, and misift_undistort_obs_batch on host arrays. */
int misift_test_adjust_bundle_radial(int max_tracks, int max_obs, const int *track_offsets, const misift_track_obs *obs,
                                     const int *export_summary, const float *points, const int *point_status,
                                     int nimages, const float *cam, const int *cam_pair, const float *intrinsics,
                                     int nhold, const int *hold, int min_views, int min_obs, int num_loops, int cg_iters,
                                     float max_error, float lambda0, int orthonormalise, int loss, float loss_scale,
                                     int ngroups, const int *group, const int *radial, const float *k0, float *cam_out,
                                     float *points_out, int *cam_obs, int *cam_status, float *cam_rms, int *point_obs,
                                     float *history, float *cost, float *obs_weight, int *summary, float *intrinsics_out,
                                     int *focal, float *radial_out);
int misift_test_undistort_obs(int max_obs, const misift_track_obs *obs, const int *export_summary, int nimages,
                              const float *intrinsics, int ngroups, const int *group, const float *radial,
                              misift_track_obs *obs_out);

/* Test-only, host-only: the whole of misift_filter_tracks_batch on host arrays, every rule compiled from the function
 * its kernels run (filter_core.hpp).  The arguments are those of the call without the context; all pointers are host;
 * no overlap check.  misift_test_filter_stage: the views of a track its wavefront stages on chip. */
int misift_test_filter_tracks(int max_tracks, int max_obs, const int *track_offsets, const misift_track_obs *obs,
                              const int *export_summary, const float *points, const int *point_status, int nimages,
                              const float *cam, const int *cam_pair, const float *intrinsics, float max_error,
                              float max_cos, int min_views, int unique_frames, int *track_offsets_out,
                              misift_track_obs *obs_out, int *export_summary_out, float *points_out,
                              int *point_views_out, int *point_status_out, int *track_map, int *obs_map, int *summary);
int misift_test_filter_stage(void);

/* Test-only, host-only: the whole of misift_merge_scenes_batch on host arrays, every rule compiled from the function its
 * kernels run (merge_core.hpp).  The arguments are those of the call without the context; all pointers are host; the
 * argument checks are the call's own.  misift_test_merge_capacity: the elements of a union its wavefront stages on chip. */
int misift_test_merge_scenes(int max_tracks_a, int max_obs_a, const int *track_offsets_a, const misift_track_obs *obs_a,
                             const int *export_summary_a, const float *points_a, const int *point_views_a,
                             const int *point_status_a, int nimages_a, const float *cam_a, const int *cam_pair_a,
                             int max_records_a, const int *record_obs_a, int max_tracks_b, int max_obs_b,
                             const int *track_offsets_b, const misift_track_obs *obs_b, const int *export_summary_b,
                             const float *points_b, const int *point_views_b, const int *point_status_b, int nimages_b,
                             const float *cam_b, const int *cam_pair_b, int max_records_b, const int *record_obs_b,
                             const int *map, const int *accept, int fshift_a, int fshift_b, int nimages_out, int rshift_a,
                             int rshift_b, int max_records_out, int max_tracks_out, int max_obs_out,
                             int *track_offsets_out, misift_track_obs *obs_out, int *export_summary_out,
                             float *points_out, int *point_views_out, int *point_status_out, float *cam_out,
                             int *cam_pair_out, int *track_map_a, int *obs_map_a, int *obs_map_b, int *record_obs_out,
                             int *summary);
int misift_test_merge_capacity(void);

/* Test-only, host-only: steps 3 and 4 of misift_resect_cameras_batch, compiled from the functions its kernels run.  The
 * sample positions: out[6 * loop + j] = position j (in the ordered list of n >= 6 candidates) of hypothesis loop after
 * srand(seed).  The six-point solve of one sample xyXYZ[5k..5k+4] = x y X Y Z of point k < 6 under intrinsics4 = fx fy cx
 * cy: cam12 = R row-major then t (twelve zeros when invalid) and *valid = 0 / 1. */
int misift_test_resect_samples(unsigned seed, int n, int num_loops, int *out);
int misift_test_resect_solve(const float *xyXYZ, const float *intrinsics4, float *cam12, int *valid);

/* Test-only, host-only: the whole of misift_describe_points_batch on host arrays, every rule compiled from the function
 * its kernel runs (localize_core.hpp).  The arguments are those of the call without the context; all pointers are host;
 * the argument checks are the call's own.
 * misift_test_localize_candidates: step 2 of misift_localize_frames_batch on one frame of nrows >= 0 host rows against T
 * points: candidate p < *out_n has out5[5p..5p+4] = x y X Y Z, out_row[p] = its row and out_track[p] = its point, in
 * ascending row order; each output holds nrows entries.  The draw and the solve are misift_test_resect_samples and
 * misift_test_resect_solve. */
int misift_test_describe_points(int max_tracks, int max_obs, const int *track_offsets, const misift_track_obs *obs,
                                const int *export_summary, const float *points, const int *point_status, const void *q,
                                int nframes, const int *counts, const int *offsets, int stride, int max_records,
                                void *scene_q, void *scene_recs, int *scene_count, int *point_members, int *summary);
int misift_test_localize_candidates(const void *rows, int nrows, int T, const float *points, const int *point_status,
                                    float min_score, float max_ambiguity, float *out5, int *out_row, int *out_track,
                                    int *out_n);

/* Test-only, host-only: steps 2, 3 and 6 of misift_align_points_batch and the arithmetic of
 * misift_transform_scene_batch, compiled from the functions their kernels run (align_core.hpp).  The sample positions:
 * out[3 * loop + j] = position j (in the ordered list of n >= 3 candidates) of hypothesis loop after srand(seed).  The
 * three-point solve of a9 = the three source points, b9 = their correspondents (x y z each): out13 = R row-major, t, s
 * (thirteen 0x7fc00000 when INVALID) and *valid = 0 / 1.  The refit: step 6 on the n candidates a3, b3 (n x 3 floats
 * each, candidate p at 3p) from the transform sim13, refitted in place, with thresh2 = thresh * thresh; the 256 slots
 * run one after another; out_counts[0] = the final members, [1] = the refits kept, *rms = the rms.  The transform of one
 * camera cam12 (R_i row-major, t_i) and of one point under sim13. */
int misift_test_align_samples(unsigned seed, int n, int num_loops, int *out);
int misift_test_align_solve(const float *a9, const float *b9, float *out13, int *valid);
int misift_test_align_refit(const float *a3, const float *b3, int n, float thresh, int refit_loops, float *sim13,
                            int *out_counts, float *rms);
int misift_test_transform_camera(const float *sim13, const float *cam12, float *out12);
int misift_test_transform_point(const float *sim13, const float *x3, float *out3);
/* Test-only, host-only: the gate and the gather of misift_match_epipolar_batch, compiled from the same headers and
 * functions as the kernel.  xy1: n1 set-1 positions (x, y), xy2: n2 set-2 positions.  gate: pass[i * n2 + j] = 1 iff
 * record j is a candidate of row i under F9 and radius.  gather: builds the cell grid of xy2 as the bin launch does
 * (grid2[0..1] = cells per axis), walks every row's band with the kernel's span functions, and sets
 * visited[i * n2 + j] = 1 iff record j lies in a cell that row i visits (0 for a non-finite position, which no cell
 * holds).  The gather is conservative iff pass & ~visited is empty. */
int misift_test_epipolar_gate(const float *F9, const float *xy1, int n1, const float *xy2, int n2, float radius,
                              unsigned char *pass);
int misift_test_epipolar_gather(const float *F9, const float *xy1, int n1, const float *xy2, int n2, float radius,
                                unsigned char *visited, int *grid2);
/* Test-only, host-only: the gate and the disc walk of misift_match_guided_batch, the walk compiled from the function
 * the kernel calls.  H9: one homography; xy1, xy2 as above.  pass[i * n2 + j] = 1 iff record j is a candidate of row i
 * (the projection in the contract's order, then ddx*ddx + ddy*ddy < fl(radius*radius)).  The cell grid of xy2 is built
 * as the bin launch builds it (grid2[0..1] = cells per axis); visited[i * n2 + j] = 1 iff record j's cell lies in the
 * cell rectangle row i walks (0 for a non-finite position, which no cell holds, and for a non-finite projection, which
 * walks nothing).  The walk is conservative iff pass & ~visited is empty. */
int misift_test_guided_gather(const float *H9, const float *xy1, int n1, const float *xy2, int n2, float radius,
                              unsigned char *pass, unsigned char *visited, int *grid2);
/* Test-only, host-only: misift_quantize_batch's rule on n floats, dst[i] = rule(src[i]).  And the work list
 * misift_match_batch_i8's plan kernel builds for pairs of n1[i] x n2[i] records on a chip of num_cus CUs: plan5[5i..5i+4] =
 * first work item, 128-row blocks, 32-column tiles, column chunks, tiles per chunk of pair i; *nitems, *chunks and
 * *partial_items_bound as for misift_test_match_batch_plan. */
int misift_test_quantize(const float *src, long n, int8_t *dst);
int misift_test_match_i8_plan(int num_cus, int npairs, const int *n1, const int *n2, int *plan5, int *nitems,
                              int *chunks, int *partial_items_bound);
/* host-only: misift_select_pairs_batch on host arrays (the rules of select_core.hpp applied with plain loops); writes
 * exactly the bytes the device call writes.  Argument errors as the device call's, but for alignment and overlap. */
int misift_test_select_pairs(const void *recs, const int8_t *q, int nframes, const int *counts, const int *offsets,
                             int stride, int top, float min_score, float max_ambiguity, int min_votes, int k,
                             int max_pairs, int *sel, int *sel_counts, int *votes, int *pairs, int *pair_votes,
                             int *summary);

/* Test-only, host-only: where the extraction calls put the pyramid inside ONE frame's arena (frame f of a batch: add
 * f * misift_scratch_floats()).  Entry i = pyramid level num_octaves - i (i = 0: the prefiltered image, or its doubled
 * form under scale_up; every next one its ScaleDown): offsets[i] = float offset of the level's first pixel, widths[i] x
 * heights[i] its size, pitches[i] its row stride in floats.  Arrays of num_octaves entries.  The table the launch sequence
 * itself is built from; the levels are still there when an extraction call has returned. */
int misift_test_pyramid_layout(int width, int height, int num_octaves, int scale_up, long long *offsets, int *widths,
                               int *heights, int *pitches);

/* Test-only, host-only: how the balanced per-keypoint launches (MISIFT_BALANCE=1) split `nblocks` workgroups among
 * `nframes` frames holding points[f] keypoints: shares[f] = 1 + floor((nblocks - nframes) * points[f] / sum), the formula
 * frame_shares_kernel evaluates on the device.  nblocks >= nframes. */
int misift_test_frame_shares(int nblocks, int nframes, const unsigned *points, int *shares);

/* Test-only: the block tables the last extraction call of this context built for its balanced per-keypoint launches.  Call
 * it once that call has completed (it copies on the context stream and waits).  *t_orient / *t_descr: the workgroups of the
 * orient_all and of the descr_all launch; rows: *t_orient + *t_descr rows of four ints, orient_all's table first — (frame,
 * sub-block, sub-blocks of the frame, 0), frame after frame, then (-1, 0, 0, 0) for the spare workgroups.  cap_rows: the
 * rows there is room for.  MISIFT_EINVAL when the last call was not balanced, or when cap_rows is too small. */
int misift_test_block_maps(misift_ctx *ctx, int *t_orient, int *t_descr, int *rows, int cap_rows);

/* Test-only, host state only (no HIP call): how a streaming launch of this context (prefilter, LowPass, ScaleDown) over
 * nframes frames of w x h pixels (row stride pitch) that writes out_w x out_rows pixels, out_lanes quads of four columns
 * per strip, is cut up under the context's CU count and knobs: out[0] = strips per row, out[1] = rows of a segment (a
 * multiple of 8 between 8 and 128 for batches), out[2] = segments per frame. */
int misift_test_strip_geom(misift_ctx *ctx, int w, int h, int pitch, int nframes, int out_w, int out_rows, int out_lanes,
                           int *out);

/* Test / tuning only: developer knobs of a context — launch shapes (segment lengths, workgroups per CU, dynamic-LDS padding)
 * and path selection (spatial binning, balanced per-keypoint launches, embedded ScaleDown chain, split pyramid tail, hipGraph
 * replay, LDS-window vs global-memory sampling, descr_big threshold ...).  Defaults are the measured optimum
 * (profiles/r05_knob_sweep.txt) and a production process never changes them: the library reads none of the corresponding
 * MISIFT_* environment variables unless MISIFT_TUNABLES=1 is set (tools/, the variant runs of the test suite).
 * misift_test_knob_names() = "knob=ENVIRONMENT_VARIABLE,..." of everything there is.  Applies to the context's pipelines
 * (misift_ctx_set_batches_in_flight) as well, also to those built later. */
int misift_test_set_knob(misift_ctx *ctx, const char *name, double value);
const char *misift_test_knob_names(void);

/* Test-only: the per-keypoint tail of the extraction calls' merged-octave sequence — spatial binning, orientations,
 * duplicate renumbering (deterministic mode), descriptors incl. the large-window kernel — on detections and pyramid
 * levels the CALLER supplies, instead of what the detector finds in an image.  The launches, their shapes (binned,
 * balanced, folded single call ...) and every buffer are those of an extraction call of `nframes` frames of width x height
 * with num_octaves octaves; the fused orientation + descriptor launch (knob fuse_orient) is never taken.
 *   scale_up != 0: the records' xpos / ypos / scale are halved as after an up-sampled call (RescalePositions); the level
 *     sizes stay those of width x height.
 *   levels[f * num_octaves + (o - 1)]: host image of octave o of frame f (o = 1: the coarsest level ... num_octaves: the
 *     finest, width x height; sizes as misift_test_pyramid_layout reports them), rows tightly packed.  The levels need
 *     not be a pyramid of one another.
 *   det_counts[f * num_octaves + (o - 1)]: detections of that frame and octave; dets: all of them in that order (frame
 *     by frame, coarsest octave first), five host floats each: xpos, ypos, scale, sharpness, edgeness in the level's own
 *     coordinates.  Finite values, scale > 0; xpos / ypos may lie outside the level.  Of an octave with more than max_pts
 *     detections the first max_pts are kept (the count stays), as the refinement does.
 *   d_pts: nframes x max_pts device records; num_pts[f] as an extraction call reports it.  The call returns when the
 *     records are complete; misift_get_counters / misift_get_counter_block then read this call's counters.
 * A bad argument returns MISIFT_EINVAL and enqueues nothing. */
int misift_test_describe_detections(misift_ctx *ctx, int nframes, int width, int height, int num_octaves, int scale_up,
                                    const float *const *levels, const float *dets, const int *det_counts, void *d_pts,
                                    int max_pts, int *num_pts);

/* Test-only: the detector of the extraction calls' merged-octave sequence — the DoG candidate scan over all levels in one
 * launch, then the refinement of its candidates — on pyramid levels the CALLER supplies, instead of what the prefilter
 * and the ScaleDown chain make of an image.  Arena, level table, candidate list, staging area, counter blocks (zeroed)
 * and every kernel argument are those of an extraction call of `nframes` frames of width x height with num_octaves
 * octaves; the scan launch never carries the embedded ScaleDown chain.  Nothing runs behind the refinement.
 *   thresh, lowest_scale: as the extraction calls take them (the octaves' scale floors are derived from lowest_scale);
 *     scale_up != 0 doubles lowest_scale as an up-sampled call does; the level sizes stay those of width x height.
 *   levels[f * num_octaves + (o - 1)]: as misift_test_describe_detections.
 *   two_ranges: 0 = one scan launch over all levels; 1 = split-tail mode's two launches, the two finest levels and then
 *     the others (num_octaves >= 3), here both on the context's stream.
 * Returned to host memory, entry k = f * num_octaves + (o - 1):
 *   cand[k * cand_slots ...]: the candidate codes the scan wrote (x | y << 14 | plane << 28, plane 0..4 = DoG plane 1..5),
 *     cand_counts[k] = min(candidates counted, the octave's list capacity) of them, in no particular order; cand_slots must
 *     hold the largest octave's capacity, max(level width * height / 4, 16384);
 *   dets[k * max_pts * 5 ...]: the staged detections, det_counts[k] = min(detections counted, max_pts) of them, five floats
 *     each: xpos, ypos, scale, sharpness, edgeness in the level's own coordinates;
 *   counters[f * 64 ...]: frame f's counter block as misift_get_counter_block reads it (uncapped counts, overflow words);
 *   scan_geom[2 * (o - 1)], [2 * (o - 1) + 1]: rows per segment and strips of 240 columns the scan cut level o into.
 * A bad argument — a call the extraction entry points would route to the dense kernels (under 16 x 16, or a coarsest
 * level under 8 pixels) included — returns MISIFT_EINVAL and enqueues nothing. */
int misift_test_detect_levels(misift_ctx *ctx, int nframes, int width, int height, int num_octaves, float thresh,
                              float lowest_scale, int scale_up, const float *const *levels, int max_pts, int two_ranges,
                              unsigned int *cand, int cand_slots, int *cand_counts, float *dets, int *det_counts,
                              unsigned int *counters, int *scan_geom);

/* Test-only: guard mode (out-of-bounds policing in the test build).  While it is on, every device
 * allocation the library makes — misift_malloc for the caller, and its own counters, candidate lists, detection staging,
 * block tables, matcher scratch, pipeline buffers — carries 64 KiB of a byte pattern in front of and behind the payload,
 * and the payload starts out filled with 0xFF (NaN as a float, -1 as an int: nothing may rely on fresh memory being zero).
 * misift_test_check_guards synchronises the device, verifies the bands of every live guarded allocation — those freed
 * since the previous check were verified as they were freed — and returns the number of damaged ones (0 = intact;
 * misift_last_error() names the first), negative on error.  MISIFT_GUARD=1 in the
 * environment switches the mode on from the first allocation.  Allocations made while the mode is off are not guarded. */
int misift_test_set_guard(int on);                 /* returns the previous mode */
int misift_test_check_guards(int *allocations);    /* allocations (optional): how many were checked */

/* Test-only, host state only (no HIP call, no synchronisation): which = 0: the bytes of the context's shared temporary
 * buffer as it stands (it only grows); which = 1: the slots of the pinned ring the batch calls copy their host lists
 * to; which = 2: the slots handed out so far (every batch call takes one, a call without a list an empty one).  MISIFT_EINVAL otherwise. */
long long misift_test_ctx_state(misift_ctx *ctx, int which);

/* ------------------------------------------------------------------- timing */

/* TimerGPU (cudautils.h:61-81): event pair on the context stream. */
int misift_timer_start(misift_ctx *ctx);
int misift_timer_stop_ms(misift_ctx *ctx, float *ms_out);

/* Per-kernel accumulated HIP-event timings of the context's launches
 * (enabled with misift_profile_enable; used by bench.py for the roofline).
 * names/ms/calls: arrays of `cap` entries; *n_out = entries filled. */
int misift_profile_enable(misift_ctx *ctx, int on);
int misift_profile_reset(misift_ctx *ctx);
int misift_profile_read(misift_ctx *ctx, int cap, char (*names)[32], float *total_ms,
                        int *calls, int *n_out);

#ifdef __cplusplus
}
#endif
#endif /* MISIFT_H */
