// surface_plan_check.cpp -- the primary-surface record in the render plan (csrc/prt_plan.h) without a device: which
// calls carry it (WavePlan::sreuse), what a pass's iteration 0 does with it (surface_form) and which kernels
// wave_schedule then names.  The expectations are data, written out per case.
//   surface_plan_check plan | schedule     one JSON line, {"ok": true, "checked": N} (failures on stderr)
//   surface_plan_check tunables            Tunables::surface_reuse / init_fold of this process's environment, one JSON line
// A deferred pass that reads the record folds the wave init into iteration 0 unless PRT_INIT_FOLD=0 (pass_init).
#include <cstdio>
#include <cstring>

#include "prt_plan.h"

using namespace prt;
using P = Pipeline;
using K = Kernel;

static int g_bad = 0;
#define CHECK(cond, ...)                        \
  do {                                           \
    if (!(cond)) {                               \
      g_bad++;                                   \
      std::fprintf(stderr, "FAIL %s: ", #cond);  \
      std::fprintf(stderr, __VA_ARGS__);         \
      std::fprintf(stderr, "\n");                \
    }                                            \
  } while (0)

// ---- a. which calls carry the record.  4,147,200 items a call is the bench's 1920x1080 x 2 frames (above the merged
// pipeline's 2^21); 8192 items is a small call, merged unless PRT_MERGE=0
struct PlanRow {
  const char* name;
  int32_t mode;
  uint32_t flags;
  int32_t bounces, spp;
  uint64_t per;
  bool area, diel;
  int32_t merge;
  bool defer, primary, shadow, surface, fold;
  Pipeline pipeline;
  bool sreuse;
  int valid_form;  // surface_form with a light-visibility record and a valid surface record
};
static const PlanRow kPlans[] = {
  {"bench frame", 0, 0x7Fu, 4, 4, 2073600ull, false, false, -1, true, true, true, true, true, P::PlainDeferred, true, kSurfInit},
  {"bench frame, PRT_INIT_FOLD=0", 0, 0x7Fu, 4, 4, 2073600ull, false, false, -1, true, true, true, true, false, P::PlainDeferred, true, kSurfRead},
  {"bench frame, per-iteration resolve", 0, 0x7Fu, 4, 4, 2073600ull, false, false, -1, false, true, true, true, true, P::Plain, true, kSurfRead},
  {"bench frame, per-iteration, PRT_INIT_FOLD=0", 0, 0x7Fu, 4, 4, 2073600ull, false, false, -1, false, true, true, true, false, P::Plain, true, kSurfRead},
  {"bench frame, PRT_SURFACE_REUSE=0", 0, 0x7Fu, 4, 4, 2073600ull, false, false, -1, true, true, true, false, true, P::PlainDeferred, false, kSurfNone},
  {"bench frame, PRT_SHADOW_REUSE=0", 0, 0x7Fu, 4, 4, 2073600ull, false, false, -1, true, true, false, true, true, P::PlainDeferred, false, kSurfNone},
  {"bench frame, PRT_PRIMARY_REUSE=0", 0, 0x7Fu, 4, 4, 2073600ull, false, false, -1, true, false, true, true, true, P::PlainDeferred, false, kSurfNone},
  {"small call", 0, 0x7Fu, 3, 4, 4096ull, false, false, -1, true, true, true, true, true, P::Merged, false, kSurfNone},
  {"small call, PRT_MERGE=0", 0, 0x7Fu, 3, 4, 4096ull, false, false, 0, true, true, true, true, true, P::PlainDeferred, true, kSurfInit},
  {"small call, PRT_MERGE=0, per-iteration", 0, 0x7Fu, 3, 4, 4096ull, false, false, 0, false, true, true, true, true, P::Plain, true, kSurfRead},
  {"small call, no AA", 0, 0x7Eu, 3, 4, 4096ull, false, false, -1, true, true, true, true, true, P::PlainDeferred, true, kSurfInit},
  {"area light", 0, 0x7Fu, 3, 4, 4096ull, true, false, 0, true, true, true, true, true, P::Ext, false, kSurfNone},
  {"dielectrics", 0, 0x7Fu, 3, 4, 4096ull, false, true, 0, true, true, true, true, true, P::Ext, false, kSurfNone},
  {"debug mode 3", 3, 0x7Fu, 3, 4, 4096ull, false, false, 0, true, true, true, true, true, P::Debug, false, kSurfNone},
  {"bounces 0", 0, 0x7Fu, 0, 4, 4096ull, false, false, 0, true, true, true, true, true, P::Plain, false, kSurfNone},
};
static WavePlan plan_of(const PlanRow& r, int& code) {
  Tunables t;
  t.merge = r.merge; t.defer = r.defer; t.primary_reuse = r.primary; t.shadow_reuse = r.shadow;
  t.surface_reuse = r.surface; t.init_fold = r.fold;
  WavePlan w;
  const char* err = "";
  code = plan_render(r.mode, r.flags, r.bounces, r.spp, r.per, r.area, r.diel, t, w, err);
  return w;
}
static int check_plan() {
  int n = 0;
  for (const PlanRow& r : kPlans) {
    int code = 0;
    const WavePlan w = plan_of(r, code);
    CHECK(code == 0, "%s: code %d", r.name, code);
    CHECK(w.pipeline == r.pipeline, "%s: pipeline %d, want %d", r.name, (int)w.pipeline, (int)r.pipeline);
    CHECK(w.sreuse == r.sreuse, "%s: sreuse %d, want %d", r.name, w.sreuse, r.sreuse);
    CHECK(!w.sreuse || (w.preuse && w.lreuse), "%s: the record rides on both reuses", r.name);
    // a pass without a light-visibility record (dense, or the record switched off) neither fills nor reads;
    // with one it fills while the surface record is stale and reads once it is valid
    CHECK(surface_form(w, false, false) == kSurfNone && surface_form(w, false, true) == kSurfNone, "%s: no lrec", r.name);
    CHECK(surface_form(w, true, false) == (r.sreuse ? kSurfFill : kSurfNone), "%s: stale", r.name);
    CHECK(surface_form(w, true, true) == r.valid_form, "%s: valid: form %d, want %d", r.name,
          surface_form(w, true, true), r.valid_form);
    // the wave init runs in front of every pass but one that folds it in
    CHECK(pass_init(kSurfNone) == K::WaveInit && pass_init(kSurfFill) == K::WaveInit &&
          pass_init(kSurfRead) == K::WaveInit && pass_init(kSurfInit) == K::None, "pass_init");
    CHECK((pass_init(surface_form(w, true, true)) == K::None) == (r.valid_form == kSurfInit), "%s: init launched", r.name);
    CHECK(pass_init(surface_form(w, true, false)) == K::WaveInit && pass_init(surface_form(w, false, true)) == K::WaveInit,
          "%s: a dense or filling pass launches the init", r.name);
    n++;
  }
  return n;
}

// ---- b. the schedule of a pass: (dense, reuse without a valid record, reuse with one) x (deferred, per-iteration)
struct SchedRow {
  Pipeline p;
  int32_t pmode;
  int lrec, surf;
  Kernel trace0, shade0;  // launch 0
};
static const SchedRow kSched[] = {
  {P::PlainDeferred, kPrimDense, 0, kSurfNone, K::Trace2Dense, K::Shade2d},
  {P::PlainDeferred, kPrimReuse, 0, kSurfNone, K::None, K::Shade2d},  // (PRT_SHADOW_REUSE=0)
  {P::PlainDeferred, kPrimReuse, 1, kSurfNone, K::None, K::Shade2dLearn},  // (PRT_SURFACE_REUSE=0)
  {P::PlainDeferred, kPrimReuse, 1, kSurfFill, K::None, K::Shade2sdFill},
  {P::PlainDeferred, kPrimReuse, 1, kSurfRead, K::None, K::Shade2sdRead},
  {P::PlainDeferred, kPrimReuse, 1, kSurfInit, K::None, K::Shade2sdInit},
  {P::Plain, kPrimDense, 0, kSurfNone, K::Trace2Dense, K::Shade2},
  {P::Plain, kPrimReuse, 0, kSurfNone, K::None, K::Shade2},
  {P::Plain, kPrimReuse, 1, kSurfNone, K::None, K::Shade2Learn},
  {P::Plain, kPrimReuse, 1, kSurfFill, K::None, K::Shade2sFill},
  {P::Plain, kPrimReuse, 1, kSurfRead, K::None, K::Shade2sRead},
};
static int check_schedule() {
  int n = 0;
  for (const SchedRow& r : kSched)
    for (uint32_t iters = 1; iters <= 3; iters++)
      for (uint32_t it = 0; it <= iters; it++) {
        const Schedule s = wave_schedule(r.p, r.lrec != 0, r.pmode, it, iters, r.surf);
        const Schedule base = wave_schedule(r.p, r.lrec != 0, r.pmode, it, iters);
        if (it == 0) {
          CHECK(s.trace == r.trace0 && s.resolve == K::None && s.shade == r.shade0,
                "pipeline %d pmode %d lrec %d surf %d iters %u: launch 0 is %d / %d / %d", (int)r.p, r.pmode, r.lrec,
                r.surf, iters, (int)s.trace, (int)s.resolve, (int)s.shade);
        } else {  // every later launch is what it was: the record changes iteration 0's shading alone
          CHECK(s.trace == base.trace && s.resolve == base.resolve && s.shade == base.shade,
                "pipeline %d pmode %d lrec %d surf %d iters %u launch %u differs", (int)r.p, r.pmode, r.lrec, r.surf,
                iters, it);
          CHECK(s.shade != K::Shade2sFill && s.shade != K::Shade2sRead && s.shade != K::Shade2sdFill &&
                s.shade != K::Shade2sdRead && s.shade != K::Shade2sdInit, "a record form behind launch 0");
        }
        CHECK(s.trace == base.trace && s.resolve == base.resolve, "the record moves no traversal or resolve launch");
        n++;
      }
  return n;
}

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!std::strcmp(mode, "tunables")) {
    const Tunables t = read_tunables();
    std::printf("{\"ok\": true, \"surface_reuse\": %d, \"init_fold\": %d, \"shadow_reuse\": %d, \"primary_reuse\": %d}\n",
                t.surface_reuse, t.init_fold, t.shadow_reuse, t.primary_reuse);
    return 0;
  }
  int n = 0;
  if (!std::strcmp(mode, "plan")) n = check_plan();
  else if (!std::strcmp(mode, "schedule")) n = check_schedule();
  else g_bad++;
  std::printf("{\"ok\": %s, \"checked\": %d}\n", g_bad ? "false" : "true", n);
  return g_bad ? 1 : 0;
}
