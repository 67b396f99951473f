// pe_layout: builds one item layout on the host and prints its counts and the
// SHA-256 of its entries (little-endian int32 quadruples: first row, rows,
// strip, flags).  No device: also the sanitizer build's driver (make asan).
//   pe_layout M N P SPEC RANK STEPS TI ORDER OVERLAP LAYOUT CAP0 CAP1 CUS [YOUNG WPERM FORCE_LAYOUT]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pe/row_classes.hpp"

namespace {

std::string sha256(const std::vector<uint8_t>& msg) {
  static const uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
      0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
      0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
      0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
      0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
      0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
      0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  std::vector<uint8_t> m = msg;
  const uint64_t bits = uint64_t(msg.size()) * 8;
  m.push_back(0x80);
  while (m.size() % 64 != 56) m.push_back(0);
  for (int i = 7; i >= 0; --i) m.push_back(uint8_t(bits >> (8 * i)));
  auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
  for (size_t off = 0; off < m.size(); off += 64) {
    uint32_t w[64];
    for (int i = 0; i < 16; ++i)
      w[i] = uint32_t(m[off + 4 * i]) << 24 | uint32_t(m[off + 4 * i + 1]) << 16 | uint32_t(m[off + 4 * i + 2]) << 8 |
             uint32_t(m[off + 4 * i + 3]);
    for (int i = 16; i < 64; ++i) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
      const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t v[8];
    for (int i = 0; i < 8; ++i) v[i] = h[i];
    for (int i = 0; i < 64; ++i) {
      const uint32_t S1 = rotr(v[4], 6) ^ rotr(v[4], 11) ^ rotr(v[4], 25), ch = (v[4] & v[5]) ^ (~v[4] & v[6]);
      const uint32_t t1 = v[7] + S1 + ch + K[i] + w[i];
      const uint32_t S0 = rotr(v[0], 2) ^ rotr(v[0], 13) ^ rotr(v[0], 22), mj = (v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]);
      for (int j = 7; j > 0; --j) v[j] = v[j - 1];
      v[4] += t1;
      v[0] = t1 + S0 + mj;
    }
    for (int i = 0; i < 8; ++i) h[i] += v[i];
  }
  char out[65];
  for (int i = 0; i < 8; ++i) std::snprintf(out + 8 * i, 9, "%08x", h[i]);
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 14) {
    std::fprintf(stderr,
                 "usage: pe_layout M N P SPEC RANK STEPS TI ORDER OVERLAP LAYOUT CAP0 CAP1 CUS [YOUNG WPERM FORCE_LAYOUT]\n");
    return 2;
  }
  pe::Problem prob;
  prob.M = std::atoi(argv[1]);
  prob.N = std::atoi(argv[2]);
  const int P = std::atoi(argv[3]);
  const pe::Block blk = pe::decompose(prob.M, prob.N, pe::process_grid_from_spec(argv[4], P, prob.M, prob.N), std::atoi(argv[5]));
  pe::LayoutRequest q;
  const int steps = std::atoi(argv[6]);
  q.ti = std::atoi(argv[7]);
  q.order = std::atoi(argv[8]);
  q.overlap = std::atoi(argv[9]) != 0;
  q.name = argv[10];
  q.wave_caps[0] = std::atoi(argv[11]);
  q.wave_caps[1] = std::atoi(argv[12]);
  q.wave_cap = std::min(q.wave_caps[0], q.wave_caps[1]);
  q.cus = std::atoi(argv[13]);
  if (argc > 14) q.knobs.young = std::atof(argv[14]);
  if (argc > 15) q.knobs.wperm = std::atoi(argv[15]);
  if (argc > 16) q.knobs.force_layout = argv[16];
  const pe::ItemLayout l = pe::block_planner(prob, blk, steps).build(q);
  std::vector<uint8_t> bytes;
  for (const pe::Entry& e : l.list)
    for (uint32_t v : {uint32_t(e.x & pe::dev::kRowMask3), uint32_t(e.y >> 20), uint32_t(e.y & 0xFFFFF),
                       uint32_t(e.x & ~pe::dev::kRowMask3)})
      for (int b = 0; b < 4; ++b) bytes.push_back(uint8_t(v >> (8 * b)));
  std::printf("name %s waves %d boundary %d cuts %d entries %zu sha256 %s\n", l.name.c_str(), l.lwaves, l.lnb[0], l.cuts,
              l.list.size(), sha256(bytes).c_str());
  return 0;
}
