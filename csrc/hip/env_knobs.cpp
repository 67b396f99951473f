// The one reader of the device runtime's PE_* environment knobs (env_knobs.hpp).
#include "env_knobs.hpp"

#include <algorithm>
#include <cstdlib>

namespace pe {

namespace {
std::optional<int> env_int(const char* name) {
  const char* e = std::getenv(name);
  return e ? std::optional<int>(std::atoi(e)) : std::nullopt;
}
std::optional<double> env_double(const char* name) {
  const char* e = std::getenv(name);
  return e ? std::optional<double>(std::atof(e)) : std::nullopt;
}
bool starts(const std::string& f, const char* prefix) { return f.rfind(prefix, 0) == 0; }

FaultInject parse_fault(const char* e) {
  FaultInject fi;
  if (!e) return fi;
  const std::string f = e;
  if (starts(f, "nan@iter:")) fi.nan_iter = std::atoll(f.c_str() + 9);
  if (starts(f, "zero@iter:")) fi.zero_iter = std::atoll(f.c_str() + 10);
  fi.stall = f == "stall";
  // stall@rank:R — only rank R hangs (its watchdog fires and aborts the
  // communicator; the peers then see the transport fail, not a hang)
  if (starts(f, "stall@rank:")) fi.stall_rank = std::atoi(f.c_str() + 11);
  // slow@rank:R,us:X — rank R's sweeps idle X µs before their cross-rank
  // sum (the peers' T_MPI must show it: iterations × X)
  if (starts(f, "slow@rank:")) {
    fi.slow_rank = std::atoi(f.c_str() + 10);
    const size_t u = f.find("us:");
    fi.slow_ticks = u == std::string::npos ? 0 : (long long)(std::atof(f.c_str() + u + 3) * 100.0);
  }
  // drift@iter:K[,amp:X] — w(M/2, N/2) += X behind the recurrence's back
  // (the end-of-solve residual check must see the gap; three-step restarts)
  if (starts(f, "drift@iter:")) {
    fi.drift = true;
    fi.drift_iter = std::atoll(f.c_str() + 11);
    const size_t u = f.find("amp:");
    if (u != std::string::npos) fi.drift_amp = std::atof(f.c_str() + u + 4);
  }
  fi.resbarrier = f == "resbarrier";
  fi.reslate = f == "reslate";
  if (starts(f, "pushtest@rank:")) fi.pushtest_rank = std::atoi(f.c_str() + 14);
  if (starts(f, "puttest@rank:")) fi.puttest_rank = std::atoi(f.c_str() + 13);
  if (starts(f, "p2ptest@rank:")) fi.p2ptest_rank = std::atoi(f.c_str() + 13);
  return fi;
}
}  // namespace

EnvKnobs read_env_knobs() {
  EnvKnobs k;
  k.plan.resident = env_int("PE_RESIDENT");
  k.plan.steps = env_int("PE_STEPS");
  k.plan.ti = env_int("PE_TI");
  k.plan.order = env_int("PE_ORDER");
  k.plan.ti_tune = env_int("PE_TI_TUNE");
  if (const char* e = std::getenv("PE_LAYOUT")) k.layout.force_layout = *e ? e : "lpt";  // (anything but equal / fill: lpt)
  if (const char* e = std::getenv("PE_YOUNG")) k.layout.young = std::max(0.5, std::atof(e));
  k.layout.wperm = env_int("PE_WPERM").value_or(0);
  // timing experiments (PE_OV_DEBUG bits): 2 serial streams, 4 natural item order (no boundary-first list)
  k.layout.ov_debug = env_int("PE_OV_DEBUG").value_or(0);
  // PE_CTOR_TRACE=1: wall time of each construction phase → stderr
  k.ctor_trace = env_int("PE_CTOR_TRACE").value_or(0);
  k.layout.trace = k.ctor_trace;
  k.fault = parse_fault(std::getenv("PE_FAULT_INJECT"));
  if (const char* e = std::getenv("PE_HALO")) k.halo = std::string(e);
  k.overlap = env_int("PE_OVERLAP");
  k.halo_tune = env_int("PE_HALO_TUNE").value_or(1) != 0;
  k.xr = env_int("PE_XR").value_or(1) != 0;
  k.push_loopback = env_int("PE_PUSH_LOOPBACK").value_or(0) == 1;
  k.put_loopback = env_int("PE_PUT_LOOPBACK").value_or(0) == 1;
  k.prio = std::max(0, std::min(20, env_int("PE_PRIO").value_or(0)));
  k.stage = env_int("PE_STAGE").value_or(1) != 0;
  k.stamps = env_int("PE_STAMPS").value_or(0) == 1;
  k.res_stamps = env_int("PE_RES_STAMPS").value_or(0) == 1;
  k.res_timeout_s = env_double("PE_RES_TIMEOUT_S");
  k.resid_gap = env_double("PE_RESID_GAP");
  k.watchdog_s = env_double("PE_WATCHDOG_S");
  k.p2p_timeout_s = env_double("PE_P2P_TIMEOUT_S");
  k.placement_tries = env_int("PE_PLACEMENT_TRIES");
  k.timer_sample = env_int("PE_TIMER_SAMPLE");
  return k;
}

}  // namespace pe
