// The PE_* environment knobs of the device runtime, parsed in one place
// (env_knobs.cpp).  read_env_knobs() reads the environment at every call —
// nothing is cached: tests change the environment between constructions within
// one process, and relayout() documents that it re-reads the layout knobs.
// An empty optional: the variable is unset.  Internal: not part of the pe/ API.
#pragma once

#include <optional>
#include <string>

#include "pe/item_layout.hpp"
#include "pe/solver_plan.hpp"

namespace pe {

// PE_FAULT_INJECT, the failure-detection hooks; one form per run.
struct FaultInject {
  long long nan_iter = 0;    // nan@iter:K — poisons the reduced sums after iteration K
  long long zero_iter = 0;   // zero@iter:K
  bool stall = false;        // stall — the host believes the device never finishes
  int stall_rank = -1;       // stall@rank:R — one rank only
  int slow_rank = -1;        // slow@rank:R,us:X — rank R's sweeps idle X µs before their cross-rank sum
  long long slow_ticks = 0;  //   X in 100 MHz ticks
  bool drift = false;        // drift@iter:K[,amp:X] — w(M/2, N/2) += X behind the recurrence's back
  long long drift_iter = 0;
  std::optional<double> drift_amp;
  bool resbarrier = false;   // resbarrier — a resident workgroup never arrives at the first grid barrier
  bool reslate = false;      // reslate — it arrives after the others have timed out
  int pushtest_rank = -1;    // pushtest@rank:R — rank R's halo-push self-test fails
  int puttest_rank = -1;     // puttest@rank:R — rank R's halo-put self-test fails
  int p2ptest_rank = -1;     // p2ptest@rank:R — rank R's P2P-sum self-test fails
};

struct EnvKnobs {
  SolverKnobs plan;          // PE_RESIDENT, PE_STEPS, PE_TI, PE_ORDER, PE_TI_TUNE
  LayoutKnobs layout;        // PE_LAYOUT, PE_YOUNG, PE_WPERM, PE_OV_DEBUG, PE_CTOR_TRACE
  int ctor_trace = 0;        // PE_CTOR_TRACE level: 1 phases, 2 every rank's halo-path split, 3 the layout's phases
  FaultInject fault;
  std::optional<std::string> halo;  // PE_HALO: exchange / put / push
  std::optional<int> overlap;       // PE_OVERLAP
  bool halo_tune = true;     // PE_HALO_TUNE=0: the first candidate, untimed
  bool xr = true;            // PE_XR=0 keeps the separate allreduce launch
  bool push_loopback = false, put_loopback = false;  // PE_PUSH_LOOPBACK=1 / PE_PUT_LOOPBACK=1 (one-GPU diagnostics)
  int prio = 0;              // PE_PRIO, 0 .. 20
  bool stage = true;         // PE_STAGE=0
  bool stamps = false;       // PE_STAMPS=1
  bool res_stamps = false;   // PE_RES_STAMPS=1
  std::optional<double> res_timeout_s;  // PE_RES_TIMEOUT_S
  std::optional<double> resid_gap;      // PE_RESID_GAP
  std::optional<double> watchdog_s;     // PE_WATCHDOG_S
  std::optional<double> p2p_timeout_s;  // PE_P2P_TIMEOUT_S
  std::optional<int> placement_tries;   // PE_PLACEMENT_TRIES
  std::optional<int> timer_sample;      // PE_TIMER_SAMPLE
};

EnvKnobs read_env_knobs();

}  // namespace pe
