// Helpers shared by the translation units of the prover (prover.cpp, prover_programs.cpp, prover_round2.cpp, prover_setup.cpp,
// prover_upload.cpp, prover_driver.cpp) and its C entry points.
#pragma once
#include "prover.h"
#include <chrono>
#include <cstdio>
#include <cstdlib>

namespace sp {

static inline double wall_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static inline bool timing_enabled() { static int v = -1; if (v < 0) v = std::getenv("SP_TIMING") ? 1 : 0; return v == 1; }
// SP_TIMING=1: wall time since the previous point on stderr (synchronises the context stream); needs `sp_ctx* ctx` and `double _tp`
#define SP_TIMEPOINT(label)                                                                 \
    do { if (timing_enabled()) { (void)hipStreamSynchronize(ctx->stream); double _t = wall_ms(); \
         std::fprintf(stderr, "[sp_timing] %-28s %9.2f ms\n", label, _t - _tp); _tp = _t; } } while (0)

// One upload block: regions in the order they are placed, each at a multiple of 256 bytes.
struct UploadLayout {
    size_t bytes = 0;
    size_t place(size_t b) { const size_t o = bytes; bytes = (bytes + b + 255) & ~size_t(255); return o; }
};
// The value table of a program (op 1 indexes it): its constants, then the RAP challenges.
static inline void fill_consts_then_rap(uint8_t* at, const std::vector<fe>& consts, const std::vector<fe>& rap) {
    fe* h = reinterpret_cast<fe*>(at);
    std::copy(consts.begin(), consts.end(), h);
    std::copy(rap.begin(), rap.end(), h + consts.size());
}

// What the main-trace builder (trace_kernels.h) reads of a run: the plan's counts, and the image's four regions where they sit on the
// device (`stage` = the device copy of the image's first byte).  trace: [plan.cols][plan.n], written by the builder.
static inline MainTraceArgs main_trace_args(const TracePlan& P, const TraceImage& I, const uint8_t* stage, fe* trace) {
    MainTraceArgs a{};
    a.regs = reinterpret_cast<const uint64_t*>(stage + I.off_regs);
    a.mem = reinterpret_cast<const fe*>(stage + I.off_mem);
    a.missing = reinterpret_cast<const uint16_t*>(stage + I.off_missing);
    a.holes = reinterpret_cast<const uint64_t*>(stage + I.off_holes);
    a.steps = P.steps; a.cells = P.mem_cells; a.n = P.n; a.r_rc = P.r_rc; a.r_holes = P.r_holes; a.r_dummy = P.r_dummy; a.n_holes = P.holes.size();
    a.rc_start = P.rc_start; a.rc_count = P.rc_count; a.cols = (uint32_t)P.cols; a.trace = trace;
    return a;
}

}  // namespace sp
