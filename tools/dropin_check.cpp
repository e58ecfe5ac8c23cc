// dropin_check — one scenario of the CudaSift drop-in API (include/cudaSift.h + include/cudaImage.h -> libcudasift.so, or
// with -DMANAGEDMEM libcudasift_managed.so) per process, for tests/test_gpu_dropin_api.py.  Built by `make` as
// build/dropin_check and build/dropin_check_managed.
//
//   dropin_check <scenario> <workdir>     reads <workdir>/in.dump, writes <workdir>/out.dump, exits 0
//   dropin_check --list                   scenario names, one per line (no GPU is touched)
//   dropin_check --poison                 the byte every output array is filled with before a call (no GPU either)
//
// A failed expectation inside the driver exits 3 with a message on stderr.  stdout belongs to the API under test
// (InitCuda, ExtractSift, MatchSiftData and PrintSiftData print there), the driver itself prints to stderr only.
//
// A dump is a sequence of entries, all little-endian:
//   u32 name length | name | u32 kind (0 int32, 1 float32, 2 bytes) | u64 payload bytes | payload
// tests/dropin_cases.py reads and writes the same format and says what every scenario's entries mean.
//
// Device memory is read back through a context of the driver's OWN (misift_ctx_create + misift_copy_d2h of
// include/misift.h), after the shim's call has returned: what any C++ caller could do.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include <unistd.h>
#include "cudaImage.h"
#include "cudaSift.h"
#include "misift.h"

static const int POISON_BYTE = 0xA5;        // = POISON_BYTE of tests/extract_capacity_cases.py (the CPU test compares them)

#ifdef MANAGEDMEM
#define HOST(d) ((d).m_data)
#define DEV(d) ((d).m_data)
static const bool MANAGED = true;
#else
#define HOST(d) ((d).h_data)
#define DEV(d) ((d).d_data)
static const bool MANAGED = false;
#endif

#define EXPECT(cond)                                                                      \
  do {                                                                                    \
    if (!(cond)) {                                                                        \
      fprintf(stderr, "dropin_check: expectation failed, line %d: %s\n", __LINE__, #cond); \
      exit(3);                                                                            \
    }                                                                                     \
  } while (0)
#define OK(call) EXPECT((call) == MISIFT_OK)

// ------------------------------------------------------------------ dumps
enum { KIND_I32 = 0, KIND_F32 = 1, KIND_BYTES = 2 };
struct Entry {
  uint32_t kind;
  std::vector<uint8_t> bytes;
};
typedef std::map<std::string, Entry> Dump;

static Dump read_dump(const std::string &path)
{
  Dump d;
  FILE *f = fopen(path.c_str(), "rb");
  EXPECT(f != NULL);
  for (;;) {
    uint32_t len = 0, kind = 0;
    uint64_t nbytes = 0;
    if (fread(&len, 4, 1, f) != 1) break;
    EXPECT(len < 256);
    std::string name(len, '\0');
    EXPECT(fread(&name[0], 1, len, f) == len);
    EXPECT(fread(&kind, 4, 1, f) == 1 && fread(&nbytes, 8, 1, f) == 1 && nbytes < (1ull << 30));
    Entry e;
    e.kind = kind;
    e.bytes.resize(nbytes);
    EXPECT(nbytes == 0 || fread(e.bytes.data(), 1, nbytes, f) == nbytes);
    d[name] = e;
  }
  fclose(f);
  return d;
}

static FILE *g_out = NULL;
static void put(const std::string &name, uint32_t kind, const void *p, size_t nbytes)
{
  const uint32_t len = (uint32_t)name.size();
  const uint64_t n = nbytes;
  fwrite(&len, 4, 1, g_out);
  fwrite(name.data(), 1, len, g_out);
  fwrite(&kind, 4, 1, g_out);
  fwrite(&n, 8, 1, g_out);
  if (nbytes) fwrite(p, 1, nbytes, g_out);
}
static void put_i(const std::string &name, int v) { put(name, KIND_I32, &v, 4); }
static void put_f(const std::string &name, const float *p, size_t n) { put(name, KIND_F32, p, 4 * n); }

static const Entry &entry(const Dump &in, const char *name)
{
  Dump::const_iterator it = in.find(name);
  if (it == in.end()) {
    fprintf(stderr, "dropin_check: in.dump has no entry '%s'\n", name);
    exit(3);
  }
  return it->second;
}
static int geti(const Dump &in, const char *name)
{
  const Entry &e = entry(in, name);
  EXPECT(e.kind == KIND_I32 && e.bytes.size() == 4);
  int v;
  memcpy(&v, e.bytes.data(), 4);
  return v;
}
static float getf(const Dump &in, const char *name)
{
  const Entry &e = entry(in, name);
  EXPECT(e.kind == KIND_F32 && e.bytes.size() == 4);
  float v;
  memcpy(&v, e.bytes.data(), 4);
  return v;
}
static std::vector<float> pixels(const Dump &in, const char *name, int w, int h)
{
  const Entry &e = entry(in, name);
  EXPECT(e.kind == KIND_F32 && e.bytes.size() == sizeof(float) * (size_t)w * h);
  std::vector<float> v((size_t)w * h);
  memcpy(v.data(), e.bytes.data(), e.bytes.size());
  return v;
}
static std::vector<SiftPoint> records(const Dump &in, const char *name)
{
  const Entry &e = entry(in, name);
  EXPECT(e.kind == KIND_BYTES && e.bytes.size() % sizeof(SiftPoint) == 0);
  std::vector<SiftPoint> v(e.bytes.size() / sizeof(SiftPoint));
  if (!v.empty()) memcpy(v.data(), e.bytes.data(), e.bytes.size());
  return v;
}

// ------------------------------------------------------------------ the driver's own context and record arrays
static misift_ctx *g_own = NULL;
static misift_ctx *own()
{
  if (!g_own) OK(misift_ctx_create(0, NULL, &g_own));
  return g_own;
}

// every byte of the host array and of the device array becomes the poison (`alloc` records: what InitSiftData was given)
static void poison(SiftData &d, int alloc)
{
  const size_t bytes = sizeof(SiftPoint) * (size_t)alloc;
  if (HOST(d)) memset(HOST(d), POISON_BYTE, bytes);
  if (!MANAGED && DEV(d)) {
    OK(misift_memset(own(), DEV(d), POISON_BYTE, bytes));
    OK(misift_ctx_sync(own()));
  }
}

// poisoned arrays with `recs` in front, on both sides, and numPts = n
static void load_set(SiftData &d, int alloc, const std::vector<SiftPoint> &recs, int n)
{
  EXPECT((int)recs.size() <= alloc && n <= (int)recs.size());
  poison(d, alloc);
  const size_t bytes = sizeof(SiftPoint) * recs.size();
  if (HOST(d) && bytes) memcpy(HOST(d), recs.data(), bytes);
  if (!MANAGED && bytes) OK(misift_copy_h2d(own(), DEV(d), recs.data(), bytes));
  d.numPts = n;
}

// <p>.numPts, <p>.maxPts, <p>.host_null, <p>.host (alloc records; absent when there is no host array) and <p>.dev
// (alloc records read through the driver's context)
static void dump_sift(const std::string &p, SiftData &d, int alloc)
{
  const size_t bytes = sizeof(SiftPoint) * (size_t)alloc;
  put_i(p + ".numPts", d.numPts);
  put_i(p + ".maxPts", d.maxPts);
  put_i(p + ".host_null", HOST(d) == NULL);
  if (HOST(d)) put(p + ".host", KIND_BYTES, HOST(d), bytes);
  std::vector<uint8_t> dev(bytes);
  OK(misift_copy_d2h(own(), dev.data(), DEV(d), bytes));
  put(p + ".dev", KIND_BYTES, dev.data(), bytes);
}

static void dump_image(const std::string &p, CudaImage &img)
{
  put_i(p + ".width", img.width);
  put_i(p + ".height", img.height);
  put_i(p + ".pitch", img.pitch);
  put_i(p + ".d_internalAlloc", img.d_internalAlloc);
  put_i(p + ".h_internalAlloc", img.h_internalAlloc);
  put_i(p + ".h_null", img.h_data == NULL);
  put_i(p + ".d_null", img.d_data == NULL);
  put_i(p + ".t_null", img.t_data == NULL);
}

struct Call {
  int w, h, noct;
  float blur, thresh;
};
static Call call_of(const Dump &in)
{
  Call c;
  c.w = geti(in, "w");
  c.h = geti(in, "h");
  c.noct = geti(in, "noct");
  c.blur = getf(in, "blur");
  c.thresh = getf(in, "thresh");
  EXPECT(c.w >= 1 && c.w <= 256 && c.h >= 1 && c.h <= 192);
  return c;
}

// ------------------------------------------------------------------ scenarios
// extract_basic, big_keypoint and chatty: the plain sequence of a caller, then Readback() into a poisoned buffer
static void basic(const Dump &in, bool match_too)
{
  const Call c = call_of(in);
  std::vector<float> px = pixels(in, "img1", c.w, c.h);
  const int alloc = 4096;
  InitCuda(0);
  CudaImage img;
  img.Allocate(c.w, c.h, iAlignUp(c.w, 128), false, NULL, px.data());
  img.Download();
  SiftData d;
  InitSiftData(d, alloc, true, true);
  float *tmp = AllocSiftTempMemory(c.w, c.h, c.noct, false);
  EXPECT(tmp != NULL);
  poison(d, alloc);
  ExtractSift(d, img, c.noct, c.blur, c.thresh, 0.0f, false, tmp);
  dump_sift("s1", d, alloc);
  dump_image("img", img);
  put_i("img.h_is_pixels", img.h_data == px.data());
  if (match_too) {
    const double ms = MatchSiftData(d, d);
    put_i("match.positive", ms > 0.0);
    dump_sift("matched", d, alloc);
  }
  const size_t n = (size_t)c.w * c.h, slack = 64;
  std::vector<float> back(n + slack);
  memset(back.data(), POISON_BYTE, sizeof(float) * back.size());
  img.h_data = back.data();                  // a public field (the reference's callers read it): borrowed, never freed
  img.Readback();
  put_f("readback", back.data(), back.size());
  img.h_data = px.data();
  FreeSiftTempMemory(tmp);
  FreeSiftData(d);
}

static void extract_lazy_ctx(const Dump &in)
{
  const Call c = call_of(in);
  std::vector<float> px = pixels(in, "img1", c.w, c.h);
  const int alloc = 4096;
  CudaImage img;                             // no InitCuda: the first call that needs the device makes the context
  img.Allocate(c.w, c.h, iAlignUp(c.w, 128), false, NULL, px.data());
  img.Download();
  SiftData d;
  InitSiftData(d, alloc, true, true);
  poison(d, alloc);
  ExtractSift(d, img, c.noct, c.blur, c.thresh);      // lowestScale = 0, scaleUp = false, tempMemory = 0
  dump_sift("s1", d, alloc);
  FreeSiftData(d);
}

static void extract_options(const Dump &in)
{
  const Call c = call_of(in);
  std::vector<float> px = pixels(in, "img1", c.w, c.h);
  const float lowest = getf(in, "lowest_scale");
  const int cap = geti(in, "cap"), alloc = 4096;
  InitCuda(0);
  CudaImage img;
  img.Allocate(c.w, c.h, iAlignUp(c.w, 128), false, NULL, px.data());
  img.Download();
  SiftData d;
  InitSiftData(d, alloc, true, true);
  float *tmp = AllocSiftTempMemory(c.w, c.h, c.noct, true);      // the larger arena: every call below fits
  poison(d, alloc);
  ExtractSift(d, img, c.noct, c.blur, c.thresh, 0.0f, true, tmp);
  dump_sift("up", d, alloc);
  poison(d, alloc);
  ExtractSift(d, img, c.noct, c.blur, c.thresh, lowest, false, tmp);
  dump_sift("low", d, alloc);
  poison(d, alloc);
  d.maxPts = cap;
  ExtractSift(d, img, c.noct, c.blur, c.thresh, 0.0f, false, tmp);
  dump_sift("cap", d, alloc);
  poison(d, alloc);
  d.maxPts = 1;
  ExtractSift(d, img, c.noct, c.blur, c.thresh, 0.0f, false, tmp);
  dump_sift("one", d, alloc);
  d.maxPts = alloc;
  FreeSiftTempMemory(tmp);
  FreeSiftData(d);
}

#ifndef MANAGEDMEM
static void extract_device_only(const Dump &in, const std::string &dir)
{
  const Call c = call_of(in);
  std::vector<float> px = pixels(in, "img1", c.w, c.h);
  const int alloc = geti(in, "max_pts");
  InitCuda(0);
  CudaImage img;
  img.Allocate(c.w, c.h, iAlignUp(c.w, 128), false, NULL, px.data());
  img.Download();
  SiftData d;
  InitSiftData(d, alloc, false, true);
  EXPECT(d.h_data == NULL && d.d_data != NULL);
  float *tmp = AllocSiftTempMemory(c.w, c.h, c.noct, false);
  poison(d, alloc);
  ExtractSift(d, img, c.noct, c.blur, c.thresh, 0.0f, false, tmp);
  dump_sift("s1", d, alloc);
  // PrintSiftData into <workdir>/print.txt
  fflush(stdout);
  const int saved = dup(1);
  FILE *f = fopen((dir + "/print.txt").c_str(), "w");
  EXPECT(saved >= 0 && f != NULL && dup2(fileno(f), 1) >= 0);
  PrintSiftData(d);
  fflush(stdout);
  EXPECT(dup2(saved, 1) >= 0);
  close(saved);
  fclose(f);
  put_i("after.host_null", d.h_data == NULL);
  put_i("after.numPts", d.numPts);
  put_i("after.maxPts", d.maxPts);
  // (PrintSiftData allocates maxPts records and fills numPts of them: the rest is not initialised, so it is not dumped)
  if (d.h_data) put("after.host", KIND_BYTES, d.h_data, sizeof(SiftPoint) * (size_t)d.numPts);
  FreeSiftTempMemory(tmp);
  FreeSiftData(d);
  put_i("freed.host_null", d.h_data == NULL);
}

static void image_ownership(const Dump &in)
{
  const Call c = call_of(in);
  std::vector<float> px = pixels(in, "img1", c.w, c.h);
  const int pitchB = geti(in, "borrowed_pitch"), offB = geti(in, "borrowed_offset"), alloc = 4096;
  EXPECT(pitchB >= c.w && pitchB % 128 != 0 && offB > 0);
  InitCuda(0);
  SiftData d;
  InitSiftData(d, alloc, true, true);
  float *tmp = AllocSiftTempMemory(c.w, c.h, c.noct, false);
  // borrowed device memory (odd pitch, d_data inside the allocation) and borrowed host memory
  const size_t poolFloats = (size_t)offB + (size_t)pitchB * c.h + 64;
  void *pool = NULL;
  OK(misift_malloc(sizeof(float) * poolFloats, &pool));
  OK(misift_memset(own(), pool, POISON_BYTE, sizeof(float) * poolFloats));
  OK(misift_ctx_sync(own()));
  std::vector<float> before(poolFloats), after(poolFloats);
  {
    CudaImage img;
    img.Allocate(c.w, c.h, pitchB, false, (float *)pool + offB, px.data());
    dump_image("borrowed", img);
    put_i("borrowed.d_is_mine", img.d_data == (float *)pool + offB);
    put_i("borrowed.h_is_mine", img.h_data == px.data());
    img.Download();
    poison(d, alloc);
    ExtractSift(d, img, c.noct, c.blur, c.thresh, 0.0f, false, tmp);
    dump_sift("borrowed.sift", d, alloc);
    OK(misift_copy_d2h(own(), before.data(), pool, sizeof(float) * poolFloats));
  }
  OK(misift_copy_d2h(own(), after.data(), pool, sizeof(float) * poolFloats));      // still readable after ~CudaImage
  put_f("pool.before", before.data(), poolFloats);
  put_f("pool.after", after.data(), poolFloats);
  put_f("pixels.after", px.data(), px.size());
  put_i("pool.free_rc", misift_free(pool));
  // owned device and host memory: the pitch passed in is replaced
  {
    CudaImage img;
    img.Allocate(c.w, c.h, 7, true);
    dump_image("owned", img);
    EXPECT(img.h_data != NULL && img.d_data != NULL && img.pitch >= c.w);
    memcpy(img.h_data, px.data(), sizeof(float) * px.size());                       // host rows are packed: stride = width
    img.Download();
    poison(d, alloc);
    ExtractSift(d, img, c.noct, c.blur, c.thresh, 0.0f, false, tmp);
    dump_sift("owned.sift", d, alloc);
    const size_t hostFloats = (size_t)img.pitch * c.h;                              // what Allocate gave h_data
    memset(img.h_data, POISON_BYTE, sizeof(float) * hostFloats);
    img.Readback();
    put_f("owned.readback", img.h_data, hostFloats);
  }
  // owned device memory, borrowed host memory
  {
    CudaImage img;
    img.Allocate(c.w, c.h, c.w, true, NULL, px.data());
    dump_image("hostmem", img);
    put_i("hostmem.h_is_mine", img.h_data == px.data());
  }
  put_f("pixels.end", px.data(), px.size());
  FreeSiftTempMemory(tmp);
  FreeSiftData(d);
}
#endif

static void demo_loop(const Dump &in)
{
  const Call c = call_of(in);
  std::vector<float> p1 = pixels(in, "img1", c.w, c.h), p2 = pixels(in, "img2", c.w, c.h);
  const int alloc = geti(in, "max_pts"), rounds = geti(in, "rounds");
  InitCuda(0);
  CudaImage img1, img2;
  img1.Allocate(c.w, c.h, iAlignUp(c.w, 128), false, NULL, p1.data());
  img2.Allocate(c.w, c.h, iAlignUp(c.w, 128), false, NULL, p2.data());
  img1.Download();
  img2.Download();
  SiftData s1, s2;
  InitSiftData(s1, alloc, true, true);
  InitSiftData(s2, alloc, true, true);
  float *tmp = AllocSiftTempMemory(c.w, c.h, c.noct, false);
  for (int r = 1; r <= rounds; r++) {
    poison(s1, alloc);
    poison(s2, alloc);
    ExtractSift(s1, img1, c.noct, c.blur, c.thresh, 0.0f, false, tmp);
    ExtractSift(s2, img2, c.noct, c.blur, c.thresh, 0.0f, false, tmp);
    if (r == 1 || r == 64 || r == rounds) {
      char name[32];
      snprintf(name, sizeof(name), "r%d.s1", r);
      dump_sift(name, s1, alloc);
      snprintf(name, sizeof(name), "r%d.s2", r);
      dump_sift(name, s2, alloc);
    }
  }
  FreeSiftTempMemory(tmp);
  FreeSiftData(s1);
  FreeSiftData(s2);
}

static void match_run(const char *name, SiftData &d1, SiftData &d2, int a1, int a2, const std::vector<SiftPoint> &r1,
                      const std::vector<SiftPoint> &r2, int n1, int n2)
{
  load_set(d1, a1, r1, n1);
  load_set(d2, a2, r2, n2);
  const double ms = MatchSiftData(d1, d2);
  const std::string p(name);
  put_i(p + ".zero", ms == 0.0);
  put_i(p + ".positive", ms > 0.0);
  dump_sift(p + ".d1", d1, a1);
  dump_sift(p + ".d2", d2, a2);
}

static void match_fields(const Dump &in)
{
  const std::vector<SiftPoint> r1 = records(in, "set1"), r2 = records(in, "set2");
  const int a1 = geti(in, "alloc1"), a2 = geti(in, "alloc2");
  const int n1 = (int)r1.size(), n2 = (int)r2.size();
  InitCuda(0);
  SiftData d1, d2;
  InitSiftData(d1, a1, true, true);
  InitSiftData(d2, a2, true, true);
  match_run("full", d1, d2, a1, a2, r1, r2, n1, n2);
  match_run("zero1", d1, d2, a1, a2, r1, r2, 0, n2);
  match_run("zero2", d1, d2, a1, a2, r1, r2, n1, 0);
  match_run("n31", d1, d2, a1, a2, r1, r2, n1, 31);
#ifndef MANAGEDMEM
  free(d1.h_data);                           // a caller that keeps set 1 on the device only
  d1.h_data = NULL;
  match_run("nohost", d1, d2, a1, a2, r1, r2, n1, n2);
#endif
  FreeSiftData(d1);
  FreeSiftData(d2);
}

static void homography(const Dump &in)
{
  const int seed = geti(in, "seed"), loops = geti(in, "loops"), iloops = geti(in, "improve_loops");
  const float minScore = getf(in, "min_score"), maxAmb = getf(in, "max_ambiguity"), thresh = getf(in, "thresh");
  const float iminScore = getf(in, "improve_min_score"), imaxAmb = getf(in, "improve_max_ambiguity"),
              ithresh = getf(in, "improve_thresh");
  InitCuda(0);
  const char *sets[2] = {"setA", "setB"};
  for (int s = 0; s < 2; s++) {
    const std::vector<SiftPoint> recs = records(in, sets[s]);
    const int n = (int)recs.size(), alloc = n + 16;
    for (int explicit_args = 0; explicit_args < 2; explicit_args++) {
      SiftData d;
      InitSiftData(d, alloc, true, true);
      load_set(d, alloc, recs, n);
      float H[9];
      int numMatches = -1;
      memset(H, POISON_BYTE, sizeof(H));
      srand((unsigned)seed);
      if (explicit_args)
        FindHomography(d, H, &numMatches, loops, minScore, maxAmb, thresh);
      else
        FindHomography(d, H, &numMatches);                      // 1000 loops, 0.85, 0.95, 5.0
      const std::string p = std::string(sets[s]) + (explicit_args ? ".explicit" : ".default");
      put_f(p + ".H_found", H, 9);
      put_i(p + ".numMatches", numMatches);
      dump_sift(p + ".found", d, alloc);
      int numfit;
      if (explicit_args)
        numfit = ImproveHomographyGPU(d, H, iloops, iminScore, imaxAmb, ithresh);
      else
        numfit = ImproveHomographyGPU(d, H, 5, 0.0f, 0.80f, 3.0f);      // the demo's arguments
      put_f(p + ".H_improved", H, 9);
      put_i(p + ".numfit", numfit);
      dump_sift(p + ".improved", d, alloc);
      FreeSiftData(d);
    }
  }
}

static void reinit(const Dump &in)
{
  const Call c = call_of(in);
  std::vector<float> px = pixels(in, "img1", c.w, c.h);
  const int alloc = 4096;
  InitCuda(0);
  CudaImage img;
  img.Allocate(c.w, c.h, iAlignUp(c.w, 128), false, NULL, px.data());
  img.Download();
  SiftData d;
  InitSiftData(d, alloc, true, true);
  float *tmp = AllocSiftTempMemory(c.w, c.h, c.noct, false);
  poison(d, alloc);
  ExtractSift(d, img, c.noct, c.blur, c.thresh, 0.0f, false, tmp);
  dump_sift("first", d, alloc);
  InitCuda(99);                              // clamped to the last device; the old context is destroyed
  poison(d, alloc);
  ExtractSift(d, img, c.noct, c.blur, c.thresh, 0.0f, false, tmp);
  dump_sift("second", d, alloc);
  const double ms = MatchSiftData(d, d);
  put_i("match.positive", ms > 0.0);
  dump_sift("matched", d, alloc);
  FreeSiftData(d);
  put_i("freed.host_null", HOST(d) == NULL);
  put_i("freed.dev_null", DEV(d) == NULL);
  put_i("freed.numPts", d.numPts);
  put_i("freed.maxPts", d.maxPts);
  FreeSiftTempMemory(tmp);
  FreeSiftTempMemory(NULL);
}

// the MANAGEDMEM build runs the scenarios in which the two flavours of the shim differ: the record arrays
static const char *SCENARIOS[] = {
  "extract_basic",
#ifndef MANAGEDMEM
  "extract_lazy_ctx", "extract_options", "extract_device_only", "image_ownership",
#endif
  "demo_loop",
#ifndef MANAGEDMEM
  "big_keypoint",
#endif
  "match_fields", "homography", "reinit",
#ifndef MANAGEDMEM
  "chatty",
#endif
};

int main(int argc, char **argv)
{
  if (argc == 2 && strcmp(argv[1], "--list") == 0) {
    for (const char *s : SCENARIOS) printf("%s\n", s);
    return 0;
  }
  if (argc == 2 && strcmp(argv[1], "--poison") == 0) {
    printf("%d\n", POISON_BYTE);
    return 0;
  }
  if (argc != 3) {
    fprintf(stderr, "usage: %s <scenario> <workdir> | --list | --poison\n", argv[0]);
    return 2;
  }
  const std::string name(argv[1]), dir(argv[2]);
  bool known = false;
  for (const char *s : SCENARIOS) known = known || name == s;
  if (!known) {
    fprintf(stderr, "dropin_check: unknown scenario '%s' (see --list)\n", argv[1]);
    return 2;
  }
  const Dump in = read_dump(dir + "/in.dump");
  g_out = fopen((dir + "/out.dump").c_str(), "wb");
  EXPECT(g_out != NULL);
  put_i("managed", MANAGED);
  put_i("poison_byte", POISON_BYTE);
  if (name == "extract_basic" || name == "big_keypoint") basic(in, false);
  else if (name == "chatty") basic(in, true);
  else if (name == "extract_lazy_ctx") extract_lazy_ctx(in);
  else if (name == "extract_options") extract_options(in);
#ifndef MANAGEDMEM
  else if (name == "extract_device_only") extract_device_only(in, dir);
  else if (name == "image_ownership") image_ownership(in);
#endif
  else if (name == "demo_loop") demo_loop(in);
  else if (name == "match_fields") match_fields(in);
  else if (name == "homography") homography(in);
  else if (name == "reinit") reinit(in);
  put_i("done", 1);
  EXPECT(fclose(g_out) == 0);
  if (g_own) misift_ctx_destroy(g_own);
  return 0;
}
