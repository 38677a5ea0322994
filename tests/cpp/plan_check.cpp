// plan_check.cpp -- the render plan (csrc/prt_plan.h) without a device: the kernels wave_schedule names for every
// launch of every pipeline, the plan plan_render chooses at the smallest inputs that flip each decision, the byte
// layout of the wavefront buffer and of the record planes, and read_tunables' parsing.  The expectations are data:
// the schedule is the table of the pipelines written out launch by launch, the plans and offsets are the values the
// render path's formulas gave before they moved into prt_plan.h.
//   plan_check schedule | select | layout      one JSON line, {"ok": true, "checked": N} (failures on stderr)
//   plan_check tunables                        the Tunables of this process's environment, one JSON line
#include <cstdio>
#include <cstring>
#include <string>

#include "prt_plan.h"

using namespace prt;
using P = Pipeline;
using K = Kernel;

static int g_bad = 0;
#define CHECK(cond, ...)                    \
  do {                                       \
    if (!(cond)) {                           \
      g_bad++;                               \
      std::fprintf(stderr, "FAIL %s: ", #cond); \
      std::fprintf(stderr, __VA_ARGS__);     \
      std::fprintf(stderr, "\n");            \
    }                                        \
  } while (0)

// ---- a. the schedule: pipeline, pmode, lrec, iters, launch -> trace, resolve stage, shade
struct SchedRow {
  Pipeline p;
  int32_t pmode;
  int lrec;
  uint32_t iters, it;
  Kernel trace, resolve, shade;
};
static const SchedRow kSched[] = {
  {P::Plain, kPrimTrace, 0, 1, 0, K::Trace2, K::None, K::Shade2},
  {P::Plain, kPrimTrace, 0, 1, 1, K::Trace2, K::Res2d, K::None},
  {P::Plain, kPrimTrace, 0, 2, 0, K::Trace2, K::None, K::Shade2},
  {P::Plain, kPrimTrace, 0, 2, 1, K::Trace2, K::Res2d, K::Shade2},
  {P::Plain, kPrimTrace, 0, 2, 2, K::Trace2, K::Res2d, K::None},
  {P::Plain, kPrimTrace, 0, 3, 0, K::Trace2, K::None, K::Shade2},
  {P::Plain, kPrimTrace, 0, 3, 1, K::Trace2, K::Res2d, K::Shade2},
  {P::Plain, kPrimTrace, 0, 3, 2, K::Trace2, K::Res2d, K::Shade2},
  {P::Plain, kPrimTrace, 0, 3, 3, K::Trace2, K::Res2d, K::None},
  {P::Plain, kPrimDense, 0, 1, 0, K::Trace2Dense, K::None, K::Shade2},
  {P::Plain, kPrimDense, 0, 1, 1, K::Trace2, K::Res2d, K::None},
  {P::Plain, kPrimDense, 0, 2, 0, K::Trace2Dense, K::None, K::Shade2},
  {P::Plain, kPrimDense, 0, 2, 1, K::Trace2, K::Res2d, K::Shade2},
  {P::Plain, kPrimDense, 0, 2, 2, K::Trace2, K::Res2d, K::None},
  {P::Plain, kPrimDense, 0, 3, 0, K::Trace2Dense, K::None, K::Shade2},
  {P::Plain, kPrimDense, 0, 3, 1, K::Trace2, K::Res2d, K::Shade2},
  {P::Plain, kPrimDense, 0, 3, 2, K::Trace2, K::Res2d, K::Shade2},
  {P::Plain, kPrimDense, 0, 3, 3, K::Trace2, K::Res2d, K::None},
  {P::Plain, kPrimReuse, 0, 1, 0, K::None, K::None, K::Shade2},
  {P::Plain, kPrimReuse, 0, 1, 1, K::Trace2, K::Res2d, K::None},
  {P::Plain, kPrimReuse, 0, 2, 0, K::None, K::None, K::Shade2},
  {P::Plain, kPrimReuse, 0, 2, 1, K::Trace2, K::Res2d, K::Shade2},
  {P::Plain, kPrimReuse, 0, 2, 2, K::Trace2, K::Res2d, K::None},
  {P::Plain, kPrimReuse, 0, 3, 0, K::None, K::None, K::Shade2},
  {P::Plain, kPrimReuse, 0, 3, 1, K::Trace2, K::Res2d, K::Shade2},
  {P::Plain, kPrimReuse, 0, 3, 2, K::Trace2, K::Res2d, K::Shade2},
  {P::Plain, kPrimReuse, 0, 3, 3, K::Trace2, K::Res2d, K::None},
  {P::Plain, kPrimReuse, 1, 1, 0, K::None, K::None, K::Shade2Learn},
  {P::Plain, kPrimReuse, 1, 1, 1, K::Trace2, K::Res2dLearn, K::None},
  {P::Plain, kPrimReuse, 1, 2, 0, K::None, K::None, K::Shade2Learn},
  {P::Plain, kPrimReuse, 1, 2, 1, K::Trace2, K::Res2dLearn, K::Shade2},
  {P::Plain, kPrimReuse, 1, 2, 2, K::Trace2, K::Res2d, K::None},
  {P::Plain, kPrimReuse, 1, 3, 0, K::None, K::None, K::Shade2Learn},
  {P::Plain, kPrimReuse, 1, 3, 1, K::Trace2, K::Res2dLearn, K::Shade2},
  {P::Plain, kPrimReuse, 1, 3, 2, K::Trace2, K::Res2d, K::Shade2},
  {P::Plain, kPrimReuse, 1, 3, 3, K::Trace2, K::Res2d, K::None},
  {P::PlainDeferred, kPrimTrace, 0, 1, 0, K::Trace2, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimTrace, 0, 1, 1, K::Trace2, K::ResolvePass, K::None},
  {P::PlainDeferred, kPrimTrace, 0, 2, 0, K::Trace2, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimTrace, 0, 2, 1, K::Trace2, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimTrace, 0, 2, 2, K::Trace2, K::ResolvePass, K::None},
  {P::PlainDeferred, kPrimTrace, 0, 3, 0, K::Trace2, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimTrace, 0, 3, 1, K::Trace2, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimTrace, 0, 3, 2, K::Trace2, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimTrace, 0, 3, 3, K::Trace2, K::ResolvePass, K::None},
  {P::PlainDeferred, kPrimDense, 0, 1, 0, K::Trace2Dense, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimDense, 0, 1, 1, K::Trace2, K::ResolvePass, K::None},
  {P::PlainDeferred, kPrimDense, 0, 2, 0, K::Trace2Dense, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimDense, 0, 2, 1, K::Trace2, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimDense, 0, 2, 2, K::Trace2, K::ResolvePass, K::None},
  {P::PlainDeferred, kPrimDense, 0, 3, 0, K::Trace2Dense, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimDense, 0, 3, 1, K::Trace2, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimDense, 0, 3, 2, K::Trace2, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimDense, 0, 3, 3, K::Trace2, K::ResolvePass, K::None},
  {P::PlainDeferred, kPrimReuse, 0, 1, 0, K::None, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimReuse, 0, 1, 1, K::Trace2, K::ResolvePass, K::None},
  {P::PlainDeferred, kPrimReuse, 0, 2, 0, K::None, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimReuse, 0, 2, 1, K::Trace2, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimReuse, 0, 2, 2, K::Trace2, K::ResolvePass, K::None},
  {P::PlainDeferred, kPrimReuse, 0, 3, 0, K::None, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimReuse, 0, 3, 1, K::Trace2, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimReuse, 0, 3, 2, K::Trace2, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimReuse, 0, 3, 3, K::Trace2, K::ResolvePass, K::None},
  {P::PlainDeferred, kPrimReuse, 1, 1, 0, K::None, K::None, K::Shade2dLearn},
  {P::PlainDeferred, kPrimReuse, 1, 1, 1, K::Trace2, K::ResolvePassLearn, K::None},
  {P::PlainDeferred, kPrimReuse, 1, 2, 0, K::None, K::None, K::Shade2dLearn},
  {P::PlainDeferred, kPrimReuse, 1, 2, 1, K::Trace2, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimReuse, 1, 2, 2, K::Trace2, K::ResolvePassLearn, K::None},
  {P::PlainDeferred, kPrimReuse, 1, 3, 0, K::None, K::None, K::Shade2dLearn},
  {P::PlainDeferred, kPrimReuse, 1, 3, 1, K::Trace2, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimReuse, 1, 3, 2, K::Trace2, K::None, K::Shade2d},
  {P::PlainDeferred, kPrimReuse, 1, 3, 3, K::Trace2, K::ResolvePassLearn, K::None},
  {P::Merged, kPrimTrace, 0, 1, 0, K::Trace2, K::None, K::Shade2m},
  {P::Merged, kPrimTrace, 0, 1, 1, K::Trace2, K::Res2md, K::None},
  {P::Merged, kPrimTrace, 0, 2, 0, K::Trace2, K::None, K::Shade2m},
  {P::Merged, kPrimTrace, 0, 2, 1, K::Trace2, K::Res2md, K::Shade2m},
  {P::Merged, kPrimTrace, 0, 2, 2, K::Trace2, K::Res2md, K::None},
  {P::Merged, kPrimTrace, 0, 3, 0, K::Trace2, K::None, K::Shade2m},
  {P::Merged, kPrimTrace, 0, 3, 1, K::Trace2, K::Res2md, K::Shade2m},
  {P::Merged, kPrimTrace, 0, 3, 2, K::Trace2, K::Res2md, K::Shade2m},
  {P::Merged, kPrimTrace, 0, 3, 3, K::Trace2, K::Res2md, K::None},
  {P::Merged, kPrimDense, 0, 1, 0, K::Trace2Dense, K::None, K::Shade2m},
  {P::Merged, kPrimDense, 0, 1, 1, K::Trace2, K::Res2md, K::None},
  {P::Merged, kPrimDense, 0, 2, 0, K::Trace2Dense, K::None, K::Shade2m},
  {P::Merged, kPrimDense, 0, 2, 1, K::Trace2, K::Res2md, K::Shade2m},
  {P::Merged, kPrimDense, 0, 2, 2, K::Trace2, K::Res2md, K::None},
  {P::Merged, kPrimDense, 0, 3, 0, K::Trace2Dense, K::None, K::Shade2m},
  {P::Merged, kPrimDense, 0, 3, 1, K::Trace2, K::Res2md, K::Shade2m},
  {P::Merged, kPrimDense, 0, 3, 2, K::Trace2, K::Res2md, K::Shade2m},
  {P::Merged, kPrimDense, 0, 3, 3, K::Trace2, K::Res2md, K::None},
  {P::Merged, kPrimReuse, 0, 1, 0, K::Trace2, K::None, K::Shade2m},
  {P::Merged, kPrimReuse, 0, 1, 1, K::Trace2, K::Res2md, K::None},
  {P::Merged, kPrimReuse, 0, 2, 0, K::Trace2, K::None, K::Shade2m},
  {P::Merged, kPrimReuse, 0, 2, 1, K::Trace2, K::Res2md, K::Shade2m},
  {P::Merged, kPrimReuse, 0, 2, 2, K::Trace2, K::Res2md, K::None},
  {P::Merged, kPrimReuse, 0, 3, 0, K::Trace2, K::None, K::Shade2m},
  {P::Merged, kPrimReuse, 0, 3, 1, K::Trace2, K::Res2md, K::Shade2m},
  {P::Merged, kPrimReuse, 0, 3, 2, K::Trace2, K::Res2md, K::Shade2m},
  {P::Merged, kPrimReuse, 0, 3, 3, K::Trace2, K::Res2md, K::None},
  {P::Merged, kPrimReuse, 1, 1, 0, K::Trace2, K::None, K::Shade2mLearn},
  {P::Merged, kPrimReuse, 1, 1, 1, K::Trace2, K::Res2mdLearn, K::None},
  {P::Merged, kPrimReuse, 1, 2, 0, K::Trace2, K::None, K::Shade2mLearn},
  {P::Merged, kPrimReuse, 1, 2, 1, K::Trace2, K::Res2mdLearn, K::Shade2m},
  {P::Merged, kPrimReuse, 1, 2, 2, K::Trace2, K::Res2md, K::None},
  {P::Merged, kPrimReuse, 1, 3, 0, K::Trace2, K::None, K::Shade2mLearn},
  {P::Merged, kPrimReuse, 1, 3, 1, K::Trace2, K::Res2mdLearn, K::Shade2m},
  {P::Merged, kPrimReuse, 1, 3, 2, K::Trace2, K::Res2md, K::Shade2m},
  {P::Merged, kPrimReuse, 1, 3, 3, K::Trace2, K::Res2md, K::None},
  {P::Ext, kPrimTrace, 0, 1, 0, K::Trace2, K::Miss2Ext, K::Shade2Ext},
  {P::Ext, kPrimTrace, 0, 1, 1, K::Trace2, K::ResMiss2Ext, K::None},
  {P::Ext, kPrimTrace, 0, 2, 0, K::Trace2, K::Miss2Ext, K::Shade2Ext},
  {P::Ext, kPrimTrace, 0, 2, 1, K::Trace2, K::ResMiss2Ext, K::Shade2Ext},
  {P::Ext, kPrimTrace, 0, 2, 2, K::Trace2, K::ResMiss2Ext, K::None},
  {P::Ext, kPrimTrace, 0, 3, 0, K::Trace2, K::Miss2Ext, K::Shade2Ext},
  {P::Ext, kPrimTrace, 0, 3, 1, K::Trace2, K::ResMiss2Ext, K::Shade2Ext},
  {P::Ext, kPrimTrace, 0, 3, 2, K::Trace2, K::ResMiss2Ext, K::Shade2Ext},
  {P::Ext, kPrimTrace, 0, 3, 3, K::Trace2, K::ResMiss2Ext, K::None},
  {P::Debug, kPrimTrace, 0, 1, 0, K::Trace2, K::Miss2, K::Shade2Debug},
  {P::Debug, kPrimTrace, 0, 1, 1, K::Trace2, K::ResMiss2, K::None},
  {P::Debug, kPrimTrace, 0, 2, 0, K::Trace2, K::Miss2, K::Shade2Debug},
  {P::Debug, kPrimTrace, 0, 2, 1, K::Trace2, K::ResMiss2, K::Shade2Debug},
  {P::Debug, kPrimTrace, 0, 2, 2, K::Trace2, K::ResMiss2, K::None},
  {P::Debug, kPrimTrace, 0, 3, 0, K::Trace2, K::Miss2, K::Shade2Debug},
  {P::Debug, kPrimTrace, 0, 3, 1, K::Trace2, K::ResMiss2, K::Shade2Debug},
  {P::Debug, kPrimTrace, 0, 3, 2, K::Trace2, K::ResMiss2, K::Shade2Debug},
  {P::Debug, kPrimTrace, 0, 3, 3, K::Trace2, K::ResMiss2, K::None},
};

static int check_schedule() {
  int n = 0;
  for (const SchedRow& r : kSched) {
    const Schedule s = wave_schedule(r.p, r.lrec != 0, r.pmode, r.it, r.iters);
    CHECK(s.trace == r.trace && s.resolve == r.resolve && s.shade == r.shade,
          "pipeline %d pmode %d lrec %d iters %u launch %u: got %d %d %d, want %d %d %d", (int)r.p, r.pmode, r.lrec, r.iters,
          r.it, (int)s.trace, (int)s.resolve, (int)s.shade, (int)r.trace, (int)r.resolve, (int)r.shade);
    n++;
  }
  // every combination that can arise is in the table: 3 pipelines x 4 (pmode, lrec) + 2 x 1, each x (2 + 3 + 4) launches
  CHECK(n == (3 * 4 + 2) * 9, "%d rows", n);
  return n;
}

// ---- b. selection
struct Tun {  // Tunables' fields that plan_render's decisions read
  int32_t merge;
  bool defer;
  uint64_t defer_budget;
  bool primary_reuse, shadow_reuse;
  uint32_t dead_shadow;
  uint64_t max_items;
};
constexpr int kUnsupported = PRT_ERR_UNSUPPORTED;
struct SelectRow {
  const char* name;
  int32_t mode;
  uint32_t flags;
  int32_t bounces, spp;
  uint64_t per;
  bool area, diel;
  Tun t;
  int code;
  const char* err;
  Pipeline pipeline;
  uint32_t iters;
  int32_t F, fmax, npass, F0;
  bool preuse, lreuse;
  uint32_t dead;
};
// plane_bytes(460800, 4) = 132710400: 126.56 MiB, the budget cases' 126 and 127
static const SelectRow kSelect[] = {
  {"mode 0", 0, 0x7Fu, 2, 4, 4096ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Merged, 3u, 2, 16384, 1, 2, true, true, 2u},
  {"mode 1", 1, 0x7Fu, 2, 4, 4096ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Debug, 4u, 2, 32768, 1, 2, false, false, 2u},
  {"no AA", 0, 0x7Eu, 2, 4, 4096ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::PlainDeferred, 2u, 4, 32768, 1, 4, true, true, 2u},
  {"bounces 0", 0, 0x7Fu, 0, 4, 4096ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Plain, 0u, 2, 32768, 1, 2, false, false, 2u},
  {"bounces 1", 0, 0x7Fu, 1, 4, 4096ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Merged, 1u, 2, 16384, 1, 2, true, true, 2u},
  {"bounces 0, no AA", 0, 0x7Eu, 0, 4, 4096ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Plain, 0u, 4, 32768, 1, 4, false, false, 2u},
  {"bounces 1, no AA", 0, 0x7Eu, 1, 4, 4096ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::PlainDeferred, 1u, 4, 32768, 1, 4, true, true, 2u},
  {"area light", 0, 0x7Fu, 2, 4, 4096ull, true, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Ext, 4u, 2, 32768, 1, 2, false, false, 2u},
  {"dielectrics", 0, 0x7Fu, 2, 4, 4096ull, false, true, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Ext, 6u, 2, 32768, 1, 2, false, false, 2u},
  {"area light + dielectrics, forced merge", 0, 0x7Fu, 2, 4, 4096ull, true, true, {1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Ext, 6u, 2, 32768, 1, 2, false, false, 2u},
  {"area light, mode 3", 3, 0x7Fu, 2, 4, 4096ull, true, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Debug, 4u, 2, 32768, 1, 2, false, false, 2u},
  {"dielectrics, mode 1", 1, 0x7Eu, 3, 4, 4096ull, false, true, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Debug, 7u, 4, 32768, 1, 4, false, false, 2u},
  {"no frames", 0, 0x7Fu, 2, 0, 4096ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Merged, 3u, 0, 16384, 1, 0, false, false, 2u},
  {"no frames, no AA", 0, 0x7Eu, 2, 0, 4096ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Plain, 2u, 0, 32768, 1, 0, false, false, 2u},
  {"no items", 0, 0x7Eu, 2, 4, 0ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Plain, 2u, 4, 134217728, 1, 4, false, false, 2u},
  {"merge unset, 2^21 items", 0, 0x7Fu, 2, 2, 2097152ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Merged, 3u, 1, 32, 1, 1, true, true, 2u},
  {"merge unset, 2^21 + 1 items", 0, 0x7Fu, 2, 2, 2097153ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::PlainDeferred, 4u, 1, 63, 1, 1, true, true, 2u},
  {"merge unset, 2^20 items x 2 frames", 0, 0x7Fu, 2, 4, 1048576ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Merged, 3u, 2, 64, 1, 2, true, true, 2u},
  {"merge unset, (2^20 + 1) items x 2 frames", 0, 0x7Fu, 2, 4, 1048577ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::PlainDeferred, 4u, 2, 127, 1, 2, true, true, 2u},
  {"PRT_MERGE=0, 2^21 items", 0, 0x7Fu, 2, 2, 2097152ull, false, false, {0, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::PlainDeferred, 4u, 1, 64, 1, 1, true, true, 2u},
  {"PRT_MERGE=0, 2^21 + 1 items", 0, 0x7Fu, 2, 2, 2097153ull, false, false, {0, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::PlainDeferred, 4u, 1, 63, 1, 1, true, true, 2u},
  {"PRT_MERGE=1, 2^21 items", 0, 0x7Fu, 2, 2, 2097152ull, false, false, {1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Merged, 3u, 1, 32, 1, 1, true, true, 2u},
  {"PRT_MERGE=1, 2^21 + 1 items", 0, 0x7Fu, 2, 2, 2097153ull, false, false, {1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Merged, 3u, 1, 31, 1, 1, true, true, 2u},
  {"PRT_MERGE=1, no AA", 0, 0x7Eu, 2, 2, 4096ull, false, false, {1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::PlainDeferred, 2u, 2, 32768, 1, 2, true, true, 2u},
  {"PRT_MERGE=1, mode 2", 2, 0x7Fu, 2, 2, 4096ull, false, false, {1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Debug, 4u, 1, 32768, 1, 1, false, false, 2u},
  {"PRT_MERGE=1, 2^26 items", 0, 0x7Fu, 2, 4, 67108864ull, false, false, {1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Merged, 3u, 2, 1, 2, 1, true, true, 2u},
  {"PRT_MERGE=1, 2^26 + 1 items", 0, 0x7Fu, 2, 4, 67108865ull, false, false, {1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Plain, 4u, 2, 1, 2, 1, true, true, 2u},
  {"2^27 items", 0, 0x7Fu, 2, 4, 134217728ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Plain, 4u, 2, 1, 2, 1, true, true, 2u},
  {"2^27 + 1 items", 0, 0x7Fu, 2, 4, 134217729ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   kUnsupported, "more than 2^27 pixels in one frame of one shard"},
  {"PRT_DEFER_RESOLVE=0", 0, 0x7Eu, 2, 4, 4096ull, false, false, {-1, false, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Plain, 2u, 4, 32768, 1, 4, true, true, 2u},
  {"PRT_DEFER_RESOLVE=0, PRT_MERGE=0", 0, 0x7Fu, 2, 4, 4096ull, false, false, {0, false, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Plain, 4u, 2, 32768, 1, 2, true, true, 2u},
  {"PRT_DEFER_RESOLVE=1, PRT_MERGE=0", 0, 0x7Fu, 2, 4, 4096ull, false, false, {0, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::PlainDeferred, 4u, 2, 32768, 1, 2, true, true, 2u},
  {"budget one MiB below the planes", 0, 0x7Eu, 4, 2, 230400ull, false, false, {-1, true, 126ull << 20, true, true, 2, 0},
   0, "", Pipeline::Plain, 4u, 2, 582, 1, 2, true, true, 2u},
  {"budget at the planes' rounded-up size", 0, 0x7Eu, 4, 2, 230400ull, false, false, {-1, true, 127ull << 20, true, true, 2, 0},
   0, "", Pipeline::PlainDeferred, 4u, 2, 582, 1, 2, true, true, 2u},
  {"budget 0", 0, 0x7Eu, 4, 2, 230400ull, false, false, {-1, true, 0ull << 20, true, true, 2, 0},
   0, "", Pipeline::Plain, 4u, 2, 582, 1, 2, true, true, 2u},
  {"PRT_PRIMARY_REUSE=0", 0, 0x7Eu, 2, 4, 4096ull, false, false, {-1, true, 4096ull << 20, false, true, 2, 0},
   0, "", Pipeline::PlainDeferred, 2u, 4, 32768, 1, 4, false, false, 2u},
  {"PRT_PRIMARY_REUSE=0, merged", 0, 0x7Fu, 2, 4, 4096ull, false, false, {-1, true, 4096ull << 20, false, true, 2, 0},
   0, "", Pipeline::Merged, 3u, 2, 16384, 1, 2, false, false, 2u},
  {"PRT_SHADOW_REUSE=0", 0, 0x7Eu, 2, 4, 4096ull, false, false, {-1, true, 4096ull << 20, true, false, 2, 0},
   0, "", Pipeline::PlainDeferred, 2u, 4, 32768, 1, 4, true, false, 2u},
  {"PRT_SHADOW_REUSE=0, area light", 0, 0x7Eu, 2, 4, 4096ull, true, false, {-1, true, 4096ull << 20, true, false, 2, 0},
   0, "", Pipeline::Ext, 2u, 4, 32768, 1, 4, false, false, 2u},
  {"PRT_DEAD_SHADOW=0", 0, 0x7Eu, 2, 4, 4096ull, false, false, {-1, true, 4096ull << 20, true, true, 0, 0},
   0, "", Pipeline::PlainDeferred, 2u, 4, 32768, 1, 4, true, true, 0u},
  {"PRT_DEAD_SHADOW=1", 0, 0x7Eu, 2, 4, 4096ull, false, false, {-1, true, 4096ull << 20, true, true, 1, 0},
   0, "", Pipeline::PlainDeferred, 2u, 4, 32768, 1, 4, true, true, 1u},
  {"PRT_DEAD_SHADOW=7", 0, 0x7Eu, 2, 4, 4096ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::PlainDeferred, 2u, 4, 32768, 1, 4, true, true, 2u},
  {"PRT_MAX_ITEMS: 1 pass", 0, 0x7Eu, 2, 6, 1000ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 6000},
   0, "", Pipeline::PlainDeferred, 2u, 6, 6, 1, 6, true, true, 2u},
  {"PRT_MAX_ITEMS: 2 passes", 0, 0x7Eu, 2, 6, 1000ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 3000},
   0, "", Pipeline::PlainDeferred, 2u, 6, 3, 2, 3, true, true, 2u},
  {"PRT_MAX_ITEMS: 3 passes", 0, 0x7Eu, 2, 6, 1000ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 2999},
   0, "", Pipeline::PlainDeferred, 2u, 6, 2, 3, 2, true, true, 2u},
  {"PRT_MAX_ITEMS below a frame", 0, 0x7Eu, 2, 6, 1000ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 999},
   0, "", Pipeline::PlainDeferred, 2u, 6, 1, 6, 1, true, true, 2u},
  {"PRT_MAX_ITEMS=0", 0, 0x7Eu, 2, 6, 1000ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 1},
   0, "", Pipeline::PlainDeferred, 2u, 6, 1, 6, 1, true, true, 2u},
  {"PRT_MAX_ITEMS: 3 merged passes of 5 frames", 0, 0x7Fu, 3, 10, 1000ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 2007},
   0, "", Pipeline::Merged, 5u, 5, 2, 3, 2, true, true, 2u},
  {"PRT_MAX_ITEMS above the merged cap", 0, 0x7Fu, 2, 4, 67108864ull, false, false, {1, true, 4096ull << 20, true, true, 2, 134217728},
   0, "", Pipeline::Merged, 3u, 2, 1, 2, 1, true, true, 2u},
  {"128 iterations", 0, 0x7Eu, 128, 1, 64ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::PlainDeferred, 128u, 1, 2097152, 1, 1, true, true, 2u},
  {"129 iterations", 0, 0x7Eu, 129, 1, 64ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   kUnsupported, "too many wavefront iterations"},
  {"64 bounces x 2 paths", 0, 0x7Fu, 64, 2, 64ull, false, false, {0, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::PlainDeferred, 128u, 1, 2097152, 1, 1, true, true, 2u},
  {"65 bounces x 2 paths", 0, 0x7Fu, 65, 2, 64ull, false, false, {0, true, 4096ull << 20, true, true, 2, 0},
   kUnsupported, "too many wavefront iterations"},
  {"65 bounces, merged", 0, 0x7Fu, 65, 2, 64ull, false, false, {-1, true, 4096ull << 20, true, true, 2, 0},
   kUnsupported, "too many wavefront iterations"},
  {"dielectrics, 6 bounces", 0, 0x7Fu, 6, 2, 64ull, false, true, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Ext, 126u, 1, 2097152, 1, 1, false, false, 2u},
  {"dielectrics, 7 bounces", 0, 0x7Fu, 7, 2, 64ull, false, true, {-1, true, 4096ull << 20, true, true, 2, 0},
   kUnsupported, "dielectric path trees exceed the wavefront iteration limit (lower bounces)"},
  {"dielectrics, 7 bounces, no AA", 0, 0x7Eu, 7, 2, 64ull, false, true, {-1, true, 4096ull << 20, true, true, 2, 0},
   0, "", Pipeline::Ext, 127u, 2, 2097152, 1, 2, false, false, 2u},
  {"dielectrics, 8 bounces", 0, 0x7Eu, 8, 2, 64ull, false, true, {-1, true, 4096ull << 20, true, true, 2, 0},
   kUnsupported, "dielectric path trees exceed the wavefront iteration limit (lower bounces)"},
  {"dielectrics, 9 bounces", 0, 0x7Eu, 9, 2, 64ull, false, true, {-1, true, 4096ull << 20, true, true, 2, 0},
   kUnsupported, "dielectric path trees exceed the wavefront iteration limit (lower bounces)"},
  {"dielectrics, 9 bounces, mode 1", 1, 0x7Eu, 9, 2, 64ull, false, true, {-1, true, 4096ull << 20, true, true, 2, 0},
   kUnsupported, "dielectric path trees exceed the wavefront iteration limit (lower bounces)"},
};

static int check_select() {
  int n = 0;
  for (const SelectRow& r : kSelect) {
    Tunables t;
    t.merge = r.t.merge; t.defer = r.t.defer; t.defer_budget = r.t.defer_budget; t.primary_reuse = r.t.primary_reuse;
    t.shadow_reuse = r.t.shadow_reuse; t.dead_shadow = r.t.dead_shadow; t.max_items = r.t.max_items;
    WavePlan w;
    const char* err = "";
    const int code = plan_render(r.mode, r.flags, r.bounces, r.spp, r.per, r.area, r.diel, t, w, err);
    CHECK(code == r.code && std::strcmp(err, r.err) == 0, "%s: code %d \"%s\", want %d \"%s\"", r.name, code, err, r.code,
          r.err);
    n++;
    if (code || r.code) continue;
    CHECK(w.pipeline == r.pipeline, "%s: pipeline %d, want %d", r.name, (int)w.pipeline, (int)r.pipeline);
    CHECK(w.iters == r.iters, "%s: iters %u, want %u", r.name, w.iters, r.iters);
    CHECK(w.F == r.F && w.fmax == r.fmax && w.npass == r.npass && w.F0 == r.F0 && w.per == r.per,
          "%s: F %d fmax %d npass %d F0 %d, want %d %d %d %d", r.name, w.F, w.fmax, w.npass, w.F0, r.F, r.fmax, r.npass, r.F0);
    CHECK(w.preuse == r.preuse && w.lreuse == r.lreuse, "%s: preuse %d lreuse %d, want %d %d", r.name, w.preuse, w.lreuse,
          r.preuse, r.lreuse);
    CHECK(w.dead == r.dead, "%s: dead %u, want %u", r.name, w.dead, r.dead);
    CHECK(w.ext() == (r.pipeline == P::Ext) && w.merge() == (r.pipeline == P::Merged) &&
          w.defer() == (r.pipeline == P::PlainDeferred), "%s: ext / merge / defer", r.name);
  }
  // the switches a plan only carries
  Tunables t;
  WavePlan w;
  const char* err = "";
  CHECK(plan_render(0, 0x7Fu, 2, 4, 4096, false, false, t, w, err) == 0 && w.coop_tail && !w.timeline, "defaults");
  t.coop_tail = false;
  t.debug_queues = true;
  CHECK(plan_render(0, 0x7Fu, 2, 4, 4096, false, false, t, w, err) == 0 && !w.coop_tail && w.timeline, "PRT_TAIL=0");
  return n + 2;
}

// ---- c. layout: offsets in the order of PRT_WAVE_ARRAYS (-1: the array is absent)
struct LayoutRow {
  uint32_t n;
  int bounces;
  bool ext, merge, needR;
  uint32_t levels, qcap, scap;
  size_t bytes;
  long long off[28];
};
static const LayoutRow kLayout[] = {
  {1u, 1, false, false, true, 1u, 256u, 1280u, 1564416ull,
   {0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304,
    2560, 2816, 3072, 3328, 3584, 36352, 69120, 232960, 233216, -1,
    -1, -1, -1, -1, -1, -1, -1, -1}},
  {257u, 3, false, false, false, 2u, 256u, 1280u, 1611520ull,
   {0, 1280, 2560, 3840, 8192, -1, 12544, 20992, 25344, 27648,
    32000, 36352, 40704, 45056, 46592, 79360, 112128, 275968, 280320, -1,
    -1, -1, -1, -1, -1, -1, -1, -1}},
  {257u, 3, true, false, true, 2u, 256u, 1280u, 1651200ull,
   {0, 1280, 2560, 3840, 8192, 12544, 20992, 29440, 33792, 36096,
    40448, 44800, 49152, 53504, 55040, 87808, 120576, 284416, 288768, -1,
    -1, -1, 1619968, 1624320, 1625600, 1634048, 1642496, 1646848}},
  {8193u, 2, false, true, true, 1u, 512u, 4096u, 4743680ull,
   {0, 33024, 66048, 131840, 263168, 394496, 656896, 919296, 1050624, 1116416,
    1247744, 1510144, 1772544, 2034944, 2100736, 2166272, 2231808, 2756096, 3018496, 4349696,
    4481024, 4612352, -1, -1, -1, -1, -1, -1}},
};
static const char* const kWaveNames[] = {"seed", "info", "rinfo", "ro", "rd", "R", "T", "s1", "jit", "hit",
                                         "ne", "nb", "nk", "vis", "q0", "q1", "shq", "hp", "ctr", "ro2",
                                         "rd2", "hit2", "na", "dst", "dro", "drd", "ao", "ad"};

static int check_layout() {
  int n = 0;
  static_assert(kWaveArrays == 28 && kW_seed == 0 && kW_R == 5 && kW_ctr == 18 && kW_ro2 == 19 && kW_na == 22 &&
                kW_ad == 27, "the order of the wavefront arrays");
  for (const LayoutRow& r : kLayout) {
    const WaveLayout L = wave_layout(r.n, r.bounces, r.ext, r.merge, r.needR);
    CHECK(L.levels == r.levels && L.qcap == r.qcap && L.scap == r.scap && L.bytes == r.bytes,
          "n %u: levels %u qcap %u scap %u bytes %zu", r.n, L.levels, L.qcap, L.scap, L.bytes);
    for (int k = 0; k < kWaveArrays; k++) {
      const long long got = L.has[k] ? (long long)L.off[k] : -1;
      CHECK(got == r.off[k], "n %u bounces %d ext %d merge %d needR %d: %s at %lld, want %lld", r.n, r.bounces, r.ext,
            r.merge, r.needR, kWaveNames[k], got, r.off[k]);
      n++;
    }
  }
  // the record planes of 257 items x 4 iterations
  static_assert(kPlaneArrays == 6 && kP_rinfo == 0 && kP_vis == 1 && kP_ne == 2 && kP_nb == 3 && kP_nk == 4 && kP_T == 5,
                "the order of the record planes");
  const size_t want[6] = {0, 4352, 8704, 25344, 41984, 58624};
  const PlaneLayout Q = plane_layout(257, 4);
  for (int k = 0; k < 6; k++, n++) CHECK(Q.off[k] == want[k], "plane %d at %zu, want %zu", k, Q.off[k], want[k]);
  CHECK(Q.bytes == 75264, "planes take %zu bytes", Q.bytes);
  CHECK(plane_layout(460800, 4).bytes == 132710400, "the budget cases' planes");
  return n;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  int n = 0;
  if (mode == "schedule") n = check_schedule();
  else if (mode == "select") n = check_select();
  else if (mode == "layout") n = check_layout();
  else if (mode == "tunables") {
    const Tunables t = read_tunables();
    std::printf("{\"ok\": true, \"merge\": %d, \"defer\": %d, \"defer_budget\": %llu, \"primary_reuse\": %d, "
                "\"shadow_reuse\": %d, \"dead_shadow\": %u, \"max_items\": %llu, \"coop_tail\": %d, \"debug_queues\": %d, "
                "\"fail_rank\": %d, \"fail_all\": %d}\n", t.merge, t.defer, (unsigned long long)t.defer_budget,
                t.primary_reuse, t.shadow_reuse, t.dead_shadow, (unsigned long long)t.max_items, t.coop_tail,
                t.debug_queues, t.fail_rank, t.fail_all);
    return 0;
  } else {
    std::fprintf(stderr, "usage: plan_check schedule|select|layout|tunables\n");
    return 2;
  }
  std::printf("{\"ok\": %s, \"checked\": %d, \"failed\": %d}\n", g_bad ? "false" : "true", n, g_bad);
  return g_bad ? 1 : 0;
}
