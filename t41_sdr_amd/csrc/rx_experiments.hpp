// t41_sdr_amd/csrc/rx_experiments.hpp -- the ONE switch behind which the diagnostic builds of the RX kernels live.
//
// The product builds with none of them (t41_sdr_amd/csrc/Makefile passes no -DT41RX_*).  A diagnostic build computes the
// product's values and writes cycle stamps or counters next to them:
//   T41RX_STAMP       per-phase cycle stamps behind the demod debug tap (tools/phase_stamps.py, tools/fc_stamps.py)
//   T41RX_PIPE_STAT   16 cycle counters per wave of the pipelined kernels, printed when the context is destroyed
//   T41RX_CLK         shader-clock and 100 MHz counter ticks per wave (tools/clock_probe.py)
// Such a build must say so: -DT41RX_EXPERIMENT=1 next to its own switch (tools/build_variant.sh passes it), otherwise this
// header stops the compilation.  The library then reports itself: every kernel object carries its own answer, and
// t41::kernel_build_flags(), their OR, is != 0 if any one of them was built so.  t41rx_create() refuses to make a context
// on such a library unless the environment says T41RX_ALLOW_EXPERIMENT=1 (rx_host.cpp), so that it cannot stand in for
// the product by accident; only then does the host honour the diagnostics' own variables (T41RX_PIPE_STAT, _STAMP_TAPS).
#pragma once

#ifndef T41RX_EXPERIMENT
#define T41RX_EXPERIMENT 0
#endif
#if defined(T41RX_STAMP) || defined(T41RX_PIPE_STAT) || defined(T41RX_CLK)
#define T41RX_DIAGNOSTICS 1
#else
#define T41RX_DIAGNOSTICS 0
#endif
#if T41RX_DIAGNOSTICS && !T41RX_EXPERIMENT
#error "T41RX_STAMP / _PIPE_STAT / _CLK are diagnostic builds: pass -DT41RX_EXPERIMENT=1 with them (rx_experiments.hpp)"
#endif

namespace t41 {
// bit 1: diagnostic stores / counters (bit 0, once timing experiments with wrong results, is no longer used)
constexpr int kKernelBuildFlags = T41RX_DIAGNOSTICS ? 2 : 0;
}  // namespace t41

// Every kernel object says what it was built as: T41RX_BUILD_FLAGS(rx512_ssb), inside namespace t41, defines the host
// function t41::build_flags_rx512_ssb() (rx_launch.hpp declares them; kernel_build_flags() is the OR of them all)
#define T41RX_BUILD_FLAGS(object) \
  int build_flags_##object() { return kKernelBuildFlags; }
