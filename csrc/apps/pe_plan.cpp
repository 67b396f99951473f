// pe_plan: the host-only solver plan of one block (pe/solver_plan.hpp), printed
// as one line.  No device: also the sanitizer build's driver (make asan).
//   pe_plan M N P SPEC RANK COMM_SIZE ALGO CUS PER_CU PER_CU0 [PE_RESIDENT PE_STEPS PE_TI PE_ORDER PE_TI_TUNE]
//           (a knob given as "-": unset)
//   pe_plan sweep   the resident tiling over nx, ny = 1 .. 140 and coarse steps to 2000 on 64 / 256 / 304 CUs, and the
//                   halo-path candidates over every combination of their inputs: counts only
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pe/solver_plan.hpp"

namespace {
std::optional<int> knob(int argc, char** argv, int i) {
  if (i >= argc || std::strcmp(argv[i], "-") == 0) return std::nullopt;
  return std::atoi(argv[i]);
}

int sweep() {
  std::vector<int64_t> v;
  for (int64_t n = 1; n <= 140; ++n) v.push_back(n);
  for (int64_t n = 1; n <= 2000; n += 53)
    if (n > 140) v.push_back(n);
  v.push_back(2000);
  long tilings = 0, rows = 0;
  for (int cus : {64, 256, 304})
    for (int64_t nx : v)
      for (int64_t ny : v)
        if (const std::optional<pe::ResidentTiling> t = pe::resident_tiling(nx, ny, cus)) {
          ++tilings;
          rows += t->rowstart.back() - t->rowstart.front();  // (= nx)
        }
  long cands = 0;
  const std::optional<std::string> halos[] = {std::nullopt, std::string("exchange"), std::string("put"), std::string("push")};
  const std::optional<int> ovs[] = {std::nullopt, 0, 1};
  for (int steps = 1; steps <= 3; ++steps)
    for (int bits = 0; bits < 8; ++bits)
      for (const auto& h : halos)
        for (const auto& o : ovs)
          for (int nh = 1; nh <= 3; ++nh)
            cands += long(pe::halo_candidates(pe::HaloInputs{steps, (bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, nh,
                                                             {48}, h, o}).list.size());
  std::printf("tilings %ld rows %ld candidates %ld\n", tilings, rows, cands);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "sweep") == 0) return sweep();
  if (argc < 11) {
    std::fprintf(stderr, "usage: pe_plan M N P SPEC RANK COMM_SIZE ALGO CUS PER_CU PER_CU0 [PE_RESIDENT PE_STEPS PE_TI PE_ORDER "
                         "PE_TI_TUNE] | pe_plan sweep\n");
    return 2;
  }
  pe::Problem prob;
  prob.M = std::atoi(argv[1]);
  prob.N = std::atoi(argv[2]);
  const int P = std::atoi(argv[3]);
  const pe::Block blk = pe::decompose(prob.M, prob.N, pe::process_grid_from_spec(argv[4], P, prob.M, prob.N), std::atoi(argv[5]));
  const int comm_size = std::atoi(argv[6]);
  pe::SolveOptions opt;
  opt.algo = std::atoi(argv[7]);
  const pe::DeviceFacts facts{std::atoi(argv[8]), std::atoi(argv[9]), std::atoi(argv[10])};
  const pe::SolverKnobs knobs{knob(argc, argv, 11), knob(argc, argv, 12), knob(argc, argv, 13), knob(argc, argv, 14),
                              knob(argc, argv, 15)};
  pe::SolverPlan pl = pe::plan_solver(prob, blk, comm_size, opt, knobs, facts.cus);
  pe::finish_plan(pl, blk, facts);
  const bool res = pl.resident_likely && pl.fused && !pl.sstep && comm_size == 1 && blk.Px * blk.Py == 1;
  const pe::ChunkPlan ch = pe::plan_chunk(pl, blk, comm_size, 0, res);
  std::string cands;
  for (int c : pl.ti_cands) cands += (cands.empty() ? "" : ",") + std::to_string(c);
  std::printf("algo %s steps %d ti %d order %d layout %s strips %lld caps %d %d tune %d [%s] slots %d chunk %d\n",
              pe::algo_name(pl.fused, pl.steps, res).c_str(), pl.steps, pl.ti, pl.order, pl.lay_name.c_str(),
              (long long)pl.geo.strips, pl.wave_caps[0], pl.wave_caps[1], int(pl.tune_ti), cands.c_str(), pl.nslot_cap, ch.chunk);
  return 0;
}
