// gfx950 (MI355X) kernels of the device-resident Jacobi-PCG solver.
//
// What the reference does per iteration (poisson_mpi_cuda2.cu:846-942):
// 5 kernels (apply_A, dot, update_w_r, apply_Dinv, dot, update_p) on a
// 16x16 block whose threadIdx.x walks the STRIDED dimension, 3 × 256 KiB of
// dot partials copied to the host and summed there, 6 device syncs, and
// a/b/B arrays streamed from HBM every time — ≈21 array passes per point.
//
// What this file does instead (8 array passes per point, 0 host syncs):
//
//   kF  (p update ⊕ stencil ⊕ 2 dots)   reads r, p_{k-1}; writes p_k
//   kG  (stop test ⊕ w,r update ⊕ recomputed stencil ⊕ (z,r) dot)
//                                        reads p_k, r, w; writes r, w
//
// Execution shape (measured: the first LDS-row version spent 85 % of its
// wave cycles in s_waitcnt/s_barrier — latency-bound, not HBM- or
// ALU-bound).  Every wave64 is independent: it owns a strip of 128
// consecutive j (2 per lane, 16-byte loads/stores) and marches down ≤ 64
// rows of i with the NEXT TWO rows' loads already in flight.  The i±1
// stencil neighbours stay in registers, j±1 come from DPP wave shifts
// (v_mov_b32_dpp wave_shl/shr:1), and the two strip-edge columns are
// computed once per work item, one row per lane, and broadcast with
// v_readlane — no LDS and no barrier inside the loop.  Work items
// (strip × row chunk) are dealt to a persistent grid.
//
// Coefficients are never stored: a per-row class table (interior interval,
// exterior hull) gives a_ij = b_ij = 1 or 1/eps with two integer compares;
// only the boundary band evaluates the fictitious-domain face lengths from
// the 1-D chord tables.  Dot products end in a deterministic last-workgroup
// reduction (agent-scope release/acquire ticket; partials summed in block
// order), so results are bitwise reproducible run to run.
#include <algorithm>

#include "kcommon.hpp"

namespace pe {
namespace dev {

namespace {

constexpr int SEG = 60;  // rows per segment: rows seg-1 .. seg+SEG live one per lane

// Per-segment lane-resident data of a strip: row classes (lane t ↔ row
// s0-1+t), strip-edge p columns (lane t ↔ row s0+t) and, for F, r of an
// in-strip halo column ny+1 (lane t ↔ row s0+t).
struct SegData {
  int4 rcv;
  double hL, hR, rup;
};

// ---------------------------------------------------------------------------
// F: p_k = D⁻¹ r_k + β p_{k-1} on owned nodes and the halo ring, then
//    S_den = Σ (A p_k)·p_k and S_pp = Σ p_k·p_k over owned nodes.
// ---------------------------------------------------------------------------
// FIELD (Problem::reaction): the row's lane pair of the reaction plane rides
// with its r / p loads (the same pitch and column origin: one aligned 16-byte
// load, issued with them) and rotates through registers as p does; the ring
// column ny+1 sits in the plane itself, the strip-edge nodes read theirs in
// p_point.
template <bool EXACT, bool SHIFT = false, bool FIELD = false>
__global__ __launch_bounds__(TJ) void kF(KParams k, int par) {
  DevState* st = k.st;
  if (st->done) return;
  __shared__ double sm[8];
  __shared__ int sflag;

  const double rz_new = (st->red_G[0] * k.h1) * k.h2;
  // Residual rule: iterate k = st->iter is tested here, at the top of
  // iteration k + 1, on the reduced (z, r) every block reads alike (NaN ≤ thr
  // is false: a non-finite g goes on to kG's tests).  One thread writes the
  // terminal state, as kG's breakdown path does; st->iter stays k.
  if (k.stop_res && k.check_tol && sqrt(rz_new) <= st->red_G[1]) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      st->rz_cur = rz_new;
      st->status = 1;
      st->done = 1;
    }
    return;
  }
  const double beta = rz_new / st->rz_cur;
  const double* __restrict__ pold = k.p[par ^ 1];
  double* __restrict__ pnew = k.p[par];
  const int64_t pitch = k.pitch;
  const int nx = int(k.nx), ny = int(k.ny);
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * kWPB;
  double sden = 0.0, spp = 0.0;

  // Wave id made provably uniform so item geometry lives in SGPRs.
  const int wid = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  for (int item = blockIdx.x * kWPB + wid; item < k.nitems; item += nw) {
    // item → (strip, row range); strip-major so a wave's consecutive items
    // continue down the same strip.
    // order 0 (default): chunk-major — concurrently running waves cover a
    // compact window of rows (TLB/L2/MALL locality); order 1: strip-major.
    const int nchunks = (nx + k.ti - 1) / k.ti;
    const int s = k.order ? item / nchunks : item % k.nstrips;
    const int ch = k.order ? item % nchunks : item / k.nstrips;
    const int j0 = 1 + s * SW;
    const int ib = 1 + ch * k.ti, ie = min(ib + k.ti - 1, nx);
    const int c0 = j0 + 2 * lane, c1 = c0 + 1;
    const int jhi = min(j0 + SW - 1, ny + 1);
    const bool own0 = c0 <= ny, own1 = c1 <= ny;
    const bool live0 = own0 || (c0 == ny + 1 && k.has[UP]);
    const bool live1 = own1 || (c1 == ny + 1 && k.has[UP]);
    const int ca = (c0 <= ny + 1) ? c0 : 1;  // clamped column for loads

    auto seg_load = [&](int s0, int s1) {
      SegData d;
      const int t = lane;
      d.rcv = (t <= s1 - s0 + 2) ? *reinterpret_cast<const int4*>(k.rowcls + (s0 + t) * 4) : make_int4(1, 0, 0, -1);
      d.hL = d.hR = d.rup = 0.0;
      if (t <= s1 - s0) {
        const int q = s0 + t;
        const int jl = j0 - 1, jr = j0 + SW;
        if (valid_node(k, q, jl)) {
          d.hL = p_point<EXACT, SHIFT, FIELD>(k, q, jl, beta, pold);
          if (jl == 0) pnew[q * pitch] = d.hL;  // rank-halo column: ours to write
        }
        if (jr <= ny + 1 && valid_node(k, q, jr)) {
          d.hR = p_point<EXACT, SHIFT, FIELD>(k, q, jr, beta, pold);
          if (jr == ny + 1) pnew[q * pitch + jr] = d.hR;
        }
      }
      if (t <= s1 - s0 + 1 && s0 + t <= nx && k.has[UP]) d.rup = k.recv_up[s0 + t - 1];
      return d;
    };

    // p(q) for both elements from r(q), p_{k-1}(q); rh = r of the halo column.
    auto prow = [&](int q, const RowCls& rc, bool fast, double2 rr, double2 po, double2 cc, double rh, double& v0,
                    double& v1) {
      const bool rin = q >= 1 && q <= nx;
      const bool rv = rin || (q == 0 && k.has[LEFT]) || (q == nx + 1 && k.has[RIGHT]);
      const double r0 = (c0 == ny + 1) ? rh : rr.x;
      const double r1 = (c1 == ny + 1) ? rh : rr.y;
      CS s0, s1;
      if (fast) {
        s0 = cset_fast<EXACT, FIELD>(k, rc, c0, cc.x);
        s1 = cset_fast<EXACT, FIELD>(k, rc, c1, cc.y);
      } else {
        const int* rcp = k.rowcls + (q + 1) * 4;
        s0 = cset<EXACT, SHIFT, FIELD>(k, rcp, q, c0, tv_at(k, ca), cc.x);
        s1 = cset<EXACT, SHIFT, FIELD>(k, rcp, q, c1, tv_at(k, ca + 1), cc.y);
      }
      const bool e0 = rv && (rin ? live0 : own0), e1 = rv && (rin ? live1 : own1);
      v0 = e0 ? zval<EXACT>(s0, r0) + beta * po.x : 0.0;
      v1 = e1 ? zval<EXACT>(s1, r1) + beta * po.y : 0.0;
    };
    auto store_row = [&](int q, double v0, double v1) {
      const bool rin = q >= 1 && q <= nx;
      const bool w0 = rin ? live0 : own0, w1 = rin ? live1 : own1;
      double* dst = pnew + q * pitch + c0;
      if (w0 && w1) *reinterpret_cast<double2*>(dst) = make_double2(v0, v1);
      else if (w0) dst[0] = v0;
    };

    const double* rptr = k.r + (ib - 1) * pitch + ca;  // row ib-1
    const double* pptr = pold + (ib - 1) * pitch + ca;
    const double2 rA = ld2(rptr), pA = ld2(pptr);
    const double2 rB = ld2(rptr + pitch), pB = ld2(pptr + pitch);
    double2 rN = ld2(rptr + 2 * pitch), pN = ld2(pptr + 2 * pitch);  // row ib+1
    rptr += 3 * pitch;                                                // → row ib+2
    pptr += 3 * pitch;
    // (FIELD) c of rows ib-1, ib, ib+1; cI: the stencil row's, cN: the next p row's
    const double2 cz = make_double2(0.0, 0.0);
    const double* cptr = nullptr;
    double2 cA = cz, cI = cz, cN = cz;
    if constexpr (FIELD) {
      cptr = k.creact + (ib - 1) * pitch + ca;
      cA = ld2(cptr);
      cI = ld2(cptr + pitch);
      cN = ld2(cptr + 2 * pitch);
      cptr += 3 * pitch;
    }
    SegData sd = seg_load(ib, min(ib + SEG - 1, ie));

    double pm0, pm1, p00, p01;
    RowCls ci = rcl_read(sd.rcv, 1);  // row ib
    bool gi = has_gen(ci, j0, jhi);
    {
      const RowCls cm = rcl_read(sd.rcv, 0);  // row ib-1
      const double rupA = (k.has[UP] && ib >= 2) ? k.recv_up[ib - 2] : 0.0;
      prow(ib - 1, cm, !has_gen(cm, j0, jhi), rA, pA, cA, rupA, pm0, pm1);
      prow(ib, ci, !gi, rB, pB, cI, readlane(sd.rup, 0), p00, p01);
    }
    if (ib == 1 && k.has[LEFT]) store_row(0, pm0, pm1);
    store_row(ib, p00, p01);

    for (int s0 = ib; s0 <= ie; s0 += SEG) {
      const int s1 = min(s0 + SEG - 1, ie);
      if (s0 != ib) sd = seg_load(s0, s1);
      // ---- march: only the prefetch stream touches vector memory ----
      for (int i = s0; i <= s1; ++i) {
        const int q = i + 1;
        const double2 rNN = ld2(rptr), pNN = ld2(pptr);  // row i+2 (≤ nx+3: padded)
        double2 cNN = cz;
        if constexpr (FIELD) {
          cNN = ld2(cptr);
          cptr += pitch;
        }
        rptr += pitch;
        pptr += pitch;

        const int rl = i - s0;
        const RowCls cq = rcl_read(sd.rcv, rl + 2);
        const bool gq = has_gen(cq, j0, jhi);
        const double rh = readlane(sd.rup, rl + 1);
        double pn0, pn1;
        prow(q, cq, !gq, rN, pN, cN, rh, pn0, pn1);
        if (q <= ie || (q == nx + 1 && k.has[RIGHT])) store_row(q, pn0, pn1);

        // j±1 neighbours of row i: DPP wave shifts, strip edges from hL/hR.
        const double eL = readlane(sd.hL, rl), eR = readlane(sd.hR, rl);
        double pl0 = dpp_shr1(p01);
        double pr1 = dpp_shl1(p00);
        if (lane == 0) pl0 = eL;
        if (lane == 63) pr1 = eR;
        CS x0, x1;
        if (!gi) {
          x0 = cset_fast<EXACT, FIELD>(k, ci, c0, cI.x);
          x1 = cset_fast<EXACT, FIELD>(k, ci, c1, cI.y);
        } else {
          const int* rcp = k.rowcls + (i + 1) * 4;
          x0 = cset<EXACT, SHIFT, FIELD>(k, rcp, i, c0, tv_at(k, ca), cI.x);
          x1 = cset<EXACT, SHIFT, FIELD>(k, rcp, i, c1, tv_at(k, ca + 1), cI.y);
        }
        const double Ap0 = stencil<EXACT, SHIFT, FIELD>(k, x0, pm0, p00, pn0, pl0, p01, cI.x);
        const double Ap1 = stencil<EXACT, SHIFT, FIELD>(k, x1, pm1, p01, pn1, p00, pr1, cI.y);
        if (own0) {
          sden += Ap0 * p00;
          spp += p00 * p00;
        }
        if (own1) {
          sden += Ap1 * p01;
          spp += p01 * p01;
        }
        pm0 = p00;
        pm1 = p01;
        p00 = pn0;
        p01 = pn1;
        rN = rNN;
        pN = pNN;
        if constexpr (FIELD) {
          cI = cN;
          cN = cNN;
        }
        ci = cq;
        gi = gq;
      }
    }
  }

  double v[2] = {sden, spp};
  block_reduce<2, false>(v, sm);
  if (threadIdx.x == 0) {
    k.partial[2 * size_t(blockIdx.x)] = v[0];
    k.partial[2 * size_t(blockIdx.x) + 1] = v[1];
  }
  if (arrive_last(&st->ticket[0], gridDim.x, &sflag)) {
    double t[2];
    reduce_partials<2>(k.partial, gridDim.x, t, sm);
    if (threadIdx.x == 0) {
      st->red_F[0] = t[0];
      st->red_F[1] = t[1];
      st->rz_cur = rz_new;
      st->beta = beta;
      __hip_atomic_store(&st->ticket[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---------------------------------------------------------------------------
// G: α = rz/den, stop test, w += α p, r -= α A p, S_zr = Σ (D⁻¹r)·r.
// ---------------------------------------------------------------------------
// FIELD: the row's c pair rides with its r / w loads (kF's note).
template <bool EXACT, bool SHIFT = false, bool FIELD = false>
__global__ __launch_bounds__(TJ) void kG(KParams k, int par) {
  DevState* st = k.st;
  if (st->done) return;
  __shared__ double sm[8];
  __shared__ int sflag;

  const double den = (st->red_F[0] * k.h1) * k.h2;
  const long long kiter = st->iter + 1;
  const bool bad = !isfinite(den) || !isfinite(st->rz_cur);
  if (bad || cg_breakdown(den, st->rz_cur, k.stop_res != 0)) {  // breakdown / non-finite: stop before touching w (reference :413)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      st->status = bad ? 4 : 2;
      st->iter = kiter;
      st->done = 1;
    }
    return;
  }
  const double alpha = st->rz_cur / den;
  const double d2 = alpha * alpha * st->red_F[1];
  const double diff = k.weighted ? sqrt((d2 * k.h1) * k.h2) : sqrt(d2);

  const double* __restrict__ p = k.p[par];
  double* __restrict__ r = k.r;
  double* __restrict__ w = k.w;
  const int64_t pitch = k.pitch;
  const int nx = int(k.nx), ny = int(k.ny);
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * kWPB;
  double szr = 0.0;

  const int wid = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  for (int item = blockIdx.x * kWPB + wid; item < k.nitems; item += nw) {
    // order 0 (default): chunk-major — concurrently running waves cover a
    // compact window of rows (TLB/L2/MALL locality); order 1: strip-major.
    const int nchunks = (nx + k.ti - 1) / k.ti;
    const int s = k.order ? item / nchunks : item % k.nstrips;
    const int ch = k.order ? item % nchunks : item / k.nstrips;
    const int j0 = 1 + s * SW;
    const int ib = 1 + ch * k.ti, ie = min(ib + k.ti - 1, nx);
    const int c0 = j0 + 2 * lane, c1 = c0 + 1;
    const int jhi = min(j0 + SW - 1, ny + 1);
    const bool own0 = c0 <= ny, own1 = c1 <= ny;
    const int ca = (c0 <= ny + 1) ? c0 : 1;

    auto seg_load = [&](int s0, int s1) {
      SegData d;
      const int t = lane;
      d.rcv = (t <= s1 - s0) ? *reinterpret_cast<const int4*>(k.rowcls + (s0 + 1 + t) * 4) : make_int4(1, 0, 0, -1);
      d.hL = d.hR = d.rup = 0.0;
      if (t <= s1 - s0) {
        const int q = s0 + t;
        d.hL = p[q * pitch + j0 - 1];
        if (j0 + SW <= ny + 1) d.hR = p[q * pitch + j0 + SW];
      }
      return d;
    };

    const double* pptr = p + (ib - 1) * pitch + ca;
    const double* rptr = r + ib * pitch + ca;
    const double* wptr = w + ib * pitch + ca;
    const double2 pA = ld2(pptr);
    double2 pB = ld2(pptr + pitch);
    double2 pN = ld2(pptr + 2 * pitch);
    double2 rC = ld2(rptr), wC = ld2(wptr);
    pptr += 3 * pitch;  // → row ib+2
    rptr += pitch;      // → row ib+1
    wptr += pitch;
    const double2 cz = make_double2(0.0, 0.0);
    const double* cptr = nullptr;
    double2 cC = cz;  // (FIELD) c of row i
    if constexpr (FIELD) {
      cptr = k.creact + ib * pitch + ca;
      cC = ld2(cptr);
      cptr += pitch;
    }
    double pm0 = pA.x, pm1 = pA.y;
    SegData sd;

    for (int s0 = ib; s0 <= ie; s0 += SEG) {
      const int s1 = min(s0 + SEG - 1, ie);
      sd = seg_load(s0, s1);
      for (int i = s0; i <= s1; ++i) {
        const double2 pNN = ld2(pptr);  // row i+2 (padded)
        const double2 rNx = ld2(rptr);  // row i+1
        const double2 wNx = ld2(wptr);
        double2 cNx = cz;
        if constexpr (FIELD) {
          cNx = ld2(cptr);  // row i+1 (padded)
          cptr += pitch;
        }
        pptr += pitch;
        rptr += pitch;
        wptr += pitch;

        const int rl = i - s0;
        const RowCls ci = rcl_read(sd.rcv, rl);
        const double eL = readlane(sd.hL, rl), eR = readlane(sd.hR, rl);
        double pl0 = dpp_shr1(pB.y);
        double pr1 = dpp_shl1(pB.x);
        if (lane == 0) pl0 = eL;
        if (lane == 63) pr1 = eR;
        CS x0, x1;
        if (!has_gen(ci, j0, jhi)) {
          x0 = cset_fast<EXACT, FIELD>(k, ci, c0, cC.x);
          x1 = cset_fast<EXACT, FIELD>(k, ci, c1, cC.y);
        } else {
          const int* rcp = k.rowcls + (i + 1) * 4;
          x0 = cset<EXACT, SHIFT, FIELD>(k, rcp, i, c0, tv_at(k, ca), cC.x);
          x1 = cset<EXACT, SHIFT, FIELD>(k, rcp, i, c1, tv_at(k, ca + 1), cC.y);
        }
        const double Ap0 = stencil<EXACT, SHIFT, FIELD>(k, x0, pm0, pB.x, pN.x, pl0, pB.y, cC.x);
        const double Ap1 = stencil<EXACT, SHIFT, FIELD>(k, x1, pm1, pB.y, pN.y, pB.x, pr1, cC.y);
        const double wn0 = wC.x + alpha * pB.x, wn1 = wC.y + alpha * pB.y;
        const double rn0 = rC.x - alpha * Ap0, rn1 = rC.y - alpha * Ap1;
        if (own0) szr += zval<EXACT>(x0, rn0) * rn0;
        if (own1) szr += zval<EXACT>(x1, rn1) * rn1;
        double* rd = r + i * pitch + c0;
        double* wd = w + i * pitch + c0;
        if (own1) {
          *reinterpret_cast<double2*>(rd) = make_double2(rn0, rn1);
          *reinterpret_cast<double2*>(wd) = make_double2(wn0, wn1);
        } else if (own0) {
          rd[0] = rn0;
          wd[0] = wn0;
        }
        if (c0 == 1 && k.has[DOWN]) k.send_dn[i - 1] = rn0;
        if (k.has[UP]) {
          if (c0 == ny) k.send_up[i - 1] = rn0;
          if (c1 == ny) k.send_up[i - 1] = rn1;
        }
        pm0 = pB.x;
        pm1 = pB.y;
        pB = pN;
        pN = pNN;
        rC = rNx;
        wC = wNx;
        if constexpr (FIELD) cC = cNx;
      }
    }
  }

  double v[1] = {szr};
  block_reduce<1, false>(v, sm);
  if (threadIdx.x == 0) k.partial[blockIdx.x] = v[0];
  if (arrive_last(&st->ticket[1], gridDim.x, &sflag)) {
    double t[1];
    reduce_partials<1>(k.partial, gridDim.x, t, sm);
    if (threadIdx.x == 0) {
      st->red_G[0] = t[0];
      if (k.fault_iter > 0 && kiter == k.fault_iter) st->rz_cur = __builtin_nan("");  // fault injection
      st->alpha = alpha;
      st->last_diff = diff;
      if (k.hist && kiter <= k.hist_n) k.hist[kiter - 1] = diff;
      st->iter = kiter;
      if (k.check_tol && !k.stop_res && diff < k.tol) {
        st->status = 1;
        st->done = 1;
      } else if (kiter >= k.max_iter) {
        st->status = 3;
        st->done = 1;
      }
      __hip_atomic_store(&st->ticket[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---------------------------------------------------------------------------
// Init: r⁰ = B - A w⁰ (w⁰ = 0 or a global-index hash), S_zr⁰ = Σ (D⁻¹r⁰)·r⁰.
// ---------------------------------------------------------------------------
template <bool EXACT, bool SHIFT = false, bool FIELD = false>
__global__ __launch_bounds__(TJ) void kInit(KParams k, int init_random, unsigned long long seed, double amp) {
  __shared__ double sm[8];
  __shared__ int sflag;
  DevState* st = k.st;
  const int64_t n = k.nx * k.ny;
  double szr = 0.0;
  for (int64_t idx = int64_t(blockIdx.x) * TJ + threadIdx.x; idx < n; idx += int64_t(gridDim.x) * TJ) {
    const int64_t li = idx / k.ny + 1, lj = idx % k.ny + 1;
    const int64_t gi = k.gi0 + li, gj = k.gj0 + lj;
    const double x = k.A1 + gi * k.h1, y = k.A2 + gj * k.h2;
    const CS c = cset_mem<EXACT, SHIFT, FIELD>(k, li, lj);
    double rr = in_ellipse(x, y, k.cx, k.cy) ? k.F : 0.0;
    const int64_t at = li * k.pitch + lj;
    double cv = 0.0;
    if constexpr (FIELD) cv = k.creact[at];
    if (init_random) {
      const double w0 = random_w0(gi, gj, k.M, k.N, seed, amp);
      const double Aw = stencil<EXACT, SHIFT, FIELD>(k, c, random_w0(gi - 1, gj, k.M, k.N, seed, amp), w0,
                                       random_w0(gi + 1, gj, k.M, k.N, seed, amp),
                                       random_w0(gi, gj - 1, k.M, k.N, seed, amp),
                                       random_w0(gi, gj + 1, k.M, k.N, seed, amp), cv);
      rr = rr - Aw;
      k.w[li * k.wpitch + lj] = w0;
    }
    k.r[at] = rr;
    if (!k.fused) {  // fused layout: launch_pack gathers the y strips
      if (lj == 1 && k.has[DOWN]) k.send_dn[li - 1] = rr;
      if (lj == k.ny && k.has[UP]) k.send_up[li - 1] = rr;
    }
    szr += zval<EXACT>(c, rr) * rr;
  }
  double v[1] = {szr};
  block_reduce<1, false>(v, sm);
  if (threadIdx.x == 0) k.partial[blockIdx.x] = v[0];
  if (arrive_last(&st->ticket[2], gridDim.x, &sflag)) {
    double t[1];
    reduce_partials<1>(k.partial, gridDim.x, t, sm);
    if (threadIdx.x == 0) {
      st->red_G[0] = t[0];
      st->rz_cur = 1.0;
      st->iter = 0;
      st->done = 0;
      st->status = 0;
      __hip_atomic_store(&st->ticket[2], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// Init from user fields (DeviceSolver::set_rhs / set_w0): kInit with B read
// from the dense nx × ny plane `Bp` (masked by the ellipse; null: F) and w⁰
// from the dense (nx+2) × (ny+2) plane `W0` (ring = the neighbours' values,
// 0 on the box boundary; null: kInit's zero / hash start).  Same stores (w
// with wpitch, r with pitch into the live layout — k.r is the classic r or
// the r-plane of x[0] behind its xorg), same sum protocol.
template <bool EXACT, bool SHIFT = false, bool FIELD = false>
__global__ __launch_bounds__(TJ) void kInitField(KParams k, const double* __restrict__ Bp,
                                                 const double* __restrict__ W0, int init_random,
                                                 unsigned long long seed, double amp) {
  __shared__ double sm[8];
  __shared__ int sflag;
  DevState* st = k.st;
  const int64_t n = k.nx * k.ny, wc = k.ny + 2;
  double szr = 0.0;
  for (int64_t idx = int64_t(blockIdx.x) * TJ + threadIdx.x; idx < n; idx += int64_t(gridDim.x) * TJ) {
    const int64_t li = idx / k.ny + 1, lj = idx % k.ny + 1;
    const int64_t gi = k.gi0 + li, gj = k.gj0 + lj;
    const double x = k.A1 + gi * k.h1, y = k.A2 + gj * k.h2;
    const CS c = cset_mem<EXACT, SHIFT, FIELD>(k, li, lj);
    double rr = in_ellipse(x, y, k.cx, k.cy) ? (Bp ? Bp[idx] : k.F) : 0.0;
    const int64_t at = li * k.pitch + lj;
    double cv = 0.0;
    if constexpr (FIELD) cv = k.creact[at];
    if (W0) {
      const int64_t q = li * wc + lj;
      const double w0 = W0[q];
      const double Aw = stencil<EXACT, SHIFT, FIELD>(k, c, W0[q - wc], w0, W0[q + wc], W0[q - 1], W0[q + 1], cv);
      rr = rr - Aw;
      k.w[li * k.wpitch + lj] = w0;
    } else if (init_random) {
      const double w0 = random_w0(gi, gj, k.M, k.N, seed, amp);
      const double Aw = stencil<EXACT, SHIFT, FIELD>(k, c, random_w0(gi - 1, gj, k.M, k.N, seed, amp), w0,
                                       random_w0(gi + 1, gj, k.M, k.N, seed, amp),
                                       random_w0(gi, gj - 1, k.M, k.N, seed, amp),
                                       random_w0(gi, gj + 1, k.M, k.N, seed, amp), cv);
      rr = rr - Aw;
      k.w[li * k.wpitch + lj] = w0;
    }
    k.r[at] = rr;
    if (!k.fused) {  // fused layout: launch_pack gathers the y strips
      if (lj == 1 && k.has[DOWN]) k.send_dn[li - 1] = rr;
      if (lj == k.ny && k.has[UP]) k.send_up[li - 1] = rr;
    }
    szr += zval<EXACT>(c, rr) * rr;
  }
  double v[1] = {szr};
  block_reduce<1, false>(v, sm);
  if (threadIdx.x == 0) k.partial[blockIdx.x] = v[0];
  if (arrive_last(&st->ticket[2], gridDim.x, &sflag)) {
    double t[1];
    reduce_partials<1>(k.partial, gridDim.x, t, sm);
    if (threadIdx.x == 0) {
      st->red_G[0] = t[0];
      st->rz_cur = 1.0;
      st->iter = 0;
      st->done = 0;
      st->status = 0;
      __hip_atomic_store(&st->ticket[2], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// A block's dense plane cut out of a global interior array in device memory
// (DeviceSolver::set_rhs_device / set_w0_device): the device twin of
// pe::block_field.  `g` is element [0][0] of the (gnx = M−1) × (gny = N−1)
// array with element strides (si, sj) ≥ 0 (0: an expanded tensor); `out` is
// rows × cols dense, rows = nx + 2 RING, cols = ny + 2 RING.  Local (li, lj)
// is global (i0−1+li, j0−1+lj); the ring holds the neighbours' values and
// exact zeros on the box boundary.  Flat grid-stride with lanes along j, so
// sj == 1 reads and all writes are coalesced; float widens exactly.
template <typename T, int RING>
__global__ __launch_bounds__(256) void kSliceField(const T* __restrict__ g, int64_t si, int64_t sj, int64_t gnx,
                                                   int64_t gny, int64_t i0, int64_t j0, int64_t rows, int64_t cols,
                                                   double* __restrict__ out) {
  const int64_t n = rows * cols;
  for (int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x; idx < n; idx += int64_t(gridDim.x) * 256) {
    const int64_t a = idx / cols, b = idx - a * cols;
    const int64_t gi = i0 + a - RING, gj = j0 + b - RING;  // global node, 1-based
    double v = 0.0;
    if (gi >= 1 && gi <= gnx && gj >= 1 && gj <= gny) v = double(g[(gi - 1) * si + (gj - 1) * sj]);
    out[idx] = v;
  }
}

// A dense (nx+2) × (ny+2) ring plane (kSliceField<T, 1>'s output, or
// pe::block_field(…, ring = 1) uploaded) into the classic p planes' layout:
// local (li, lj) at dst + li·pitch + lj (DeviceSolver::set_reaction*: the
// reaction plane the FIELD kernels load next to p).  Padding stays as allocated (0).
__global__ __launch_bounds__(256) void kRingToPitched(const double* __restrict__ src, int64_t rows, int64_t cols,
                                                      double* __restrict__ dst, int64_t pitch) {
  const int64_t n = rows * cols;
  for (int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x; idx < n; idx += int64_t(gridDim.x) * 256) {
    const int64_t a = idx / cols, b = idx - a * cols;
    dst[a * pitch + b] = src[idx];
  }
}

// The owned nx × ny part of w (either layout: local (li, lj) at
// w + li·wpitch + lj) into a destination with element strides (si, sj), at
// element offset (off_i, off_j): (0, 0) for a dense block, (i0−1, j0−1) for
// the block's position inside a global interior array
// (DeviceSolver::copy_w_device, after the deferred w term is flushed).
__global__ __launch_bounds__(256) void kGatherW(const double* __restrict__ w, int64_t wpitch, int64_t nx, int64_t ny,
                                                double* __restrict__ dst, int64_t si, int64_t sj, int64_t off_i,
                                                int64_t off_j) {
  const int64_t n = nx * ny;
  for (int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x; idx < n; idx += int64_t(gridDim.x) * 256) {
    const int64_t li = idx / ny, lj = idx - li * ny;
    dst[(off_i + li) * si + (off_j + lj) * sj] = w[(li + 1) * wpitch + lj + 1];
  }
}

// Error against the analytic solution u = F(1 - cx x² - cy y²)/(2cx + 2cy),
// or (FIELD) against the user's exact solution read from the dense nx × ny
// plane `Up` (DeviceSolver::set_exact; values outside the ellipse are never
// read).  Same walk, mask, block-ordered reduction and st->err slots either way.
template <bool FIELD>
__device__ __forceinline__ void error_body(const KParams& k, const double* Up) {
  __shared__ double sm[8];
  __shared__ int sflag;
  DevState* st = k.st;
  const int64_t n = k.nx * k.ny;
  double e2 = 0.0, emax = 0.0, omax = 0.0;
  for (int64_t idx = int64_t(blockIdx.x) * TJ + threadIdx.x; idx < n; idx += int64_t(gridDim.x) * TJ) {
    const int64_t li = idx / k.ny + 1, lj = idx % k.ny + 1;
    const double x = k.A1 + (k.gi0 + li) * k.h1, y = k.A2 + (k.gj0 + lj) * k.h2;
    const double wv = k.w[li * k.wpitch + lj];
    if (in_ellipse(x, y, k.cx, k.cy)) {
      const double e = wv - (FIELD ? Up[idx] : k.u_scale * (1.0 - k.cx * x * x - k.cy * y * y));
      e2 += e * e;
      emax = fmax(emax, fabs(e));
    } else {
      omax = fmax(omax, fabs(wv));
    }
  }
  double s[1] = {e2};
  double m[2] = {emax, omax};
  block_reduce<1, false>(s, sm);
  __syncthreads();
  block_reduce<2, true>(m, sm);
  if (threadIdx.x == 0) {
    k.partial[3 * size_t(blockIdx.x)] = s[0];
    k.partial[3 * size_t(blockIdx.x) + 1] = m[0];
    k.partial[3 * size_t(blockIdx.x) + 2] = m[1];
  }
  if (arrive_last(&st->ticket[3], gridDim.x, &sflag)) {
    double acc = 0.0, m0 = 0.0, m1 = 0.0;
    for (unsigned b = threadIdx.x; b < gridDim.x; b += TJ) {
      acc += k.partial[3 * size_t(b)];
      m0 = fmax(m0, k.partial[3 * size_t(b) + 1]);
      m1 = fmax(m1, k.partial[3 * size_t(b) + 2]);
    }
    double s2[1] = {acc};
    double mm[2] = {m0, m1};
    block_reduce<1, false>(s2, sm);
    __syncthreads();
    block_reduce<2, true>(mm, sm);
    if (threadIdx.x == 0) {
      st->err[0] = s2[0];
      st->err[1] = mm[0];
      st->err[2] = mm[1];
      __hip_atomic_store(&st->ticket[3], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
__global__ __launch_bounds__(TJ) void kError(KParams k) { error_body<false>(k, nullptr); }
__global__ __launch_bounds__(TJ) void kErrorField(KParams k, const double* __restrict__ Up) {
  error_body<true>(k, Up);
}

// True-residual check of a single-sweep-layout solve (DeviceSolver::residual_pass):
// ρ = B − A w on the owned nodes, w read from the p-plane of x[bw] (kWtoP
// copied it there and the sweep's halo exchange filled its halo), the
// recurrence's r from the r-plane of x[st->wpar] (with_r).  Unweighted sums
// into st->res = {Σρ², Σr², Σ(ρ − r)², ΣB²}, block partials summed
// in block order (deterministic).  store: ρ → the r-plane of x[bw] (the
// three-step restart's r⁰; this kernel reads no r there).
// Bp: the user right-hand side's dense nx × ny plane (FIELD; masked by the
// ellipse like F), so the check — and the three-step restart's stored ρ —
// belong to the user's problem.
template <bool FIELD>
__device__ __forceinline__ void resid_body(const KParams& k, int bw, int with_r, int store, const double* Bp) {
  __shared__ double sm[16];
  __shared__ int sflag;
  DevState* st = k.st;
  const int64_t n = k.nx * k.ny;
  const double* wv = k.x[bw] + k.poff;
  const double* xr = k.x[with_r ? st->wpar : bw];
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t idx = int64_t(blockIdx.x) * TJ + threadIdx.x; idx < n; idx += int64_t(gridDim.x) * TJ) {
    const int64_t li = idx / k.ny + 1, lj = idx % k.ny + 1;
    const double x = k.A1 + (k.gi0 + li) * k.h1, y = k.A2 + (k.gj0 + lj) * k.h2;
    const CS c = cset_mem<false>(k, li, lj);
    const int64_t at = li * k.pitch + lj;
    const double B = in_ellipse(x, y, k.cx, k.cy) ? (FIELD ? Bp[idx] : k.F) : 0.0;
    const double rho = B - stencil<false>(k, c, wv[at - k.pitch], wv[at], wv[at + k.pitch], wv[at - 1], wv[at + 1]);
    a[0] += rho * rho;
    a[3] += B * B;
    if (with_r) {
      const double r = xr[at];
      a[1] += r * r;
      a[2] += (rho - r) * (rho - r);
    }
    if (store) k.x[bw][at] = rho;
  }
  block_reduce<4, false>(a, sm);
  if (threadIdx.x == 0)
#pragma unroll
    for (int q = 0; q < 4; ++q) k.partial[4 * size_t(blockIdx.x) + q] = a[q];
  if (arrive_last(&st->ticket[3], gridDim.x, &sflag)) {
    double t[4];
    reduce_partials<4>(k.partial, gridDim.x, t, sm);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) st->res[q] = t[q];
      __hip_atomic_store(&st->ticket[3], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
__global__ __launch_bounds__(TJ) void kResid(KParams k, int bw, int with_r, int store) {
  resid_body<false>(k, bw, with_r, store, nullptr);
}
__global__ __launch_bounds__(TJ) void kResidField(KParams k, int bw, int with_r, int store,
                                                  const double* __restrict__ Bp) {
  resid_body<true>(k, bw, with_r, store, Bp);
}

// w (owned nodes) → the p-plane of x[b] (kResid's operand).
__global__ __launch_bounds__(TJ) void kWtoP(KParams k, int b) {
  const int64_t n = k.nx * k.ny;
  double* dst = k.x[b] + k.poff;
  for (int64_t idx = int64_t(blockIdx.x) * TJ + threadIdx.x; idx < n; idx += int64_t(gridDim.x) * TJ) {
    const int64_t li = idx / k.ny + 1, lj = idx % k.ny + 1;
    dst[li * k.pitch + lj] = k.w[li * k.wpitch + lj];
  }
}

// Classic layout, before kGradField: owned w → the r plane, its first and last
// columns → send_dn / send_up — what halo_plan() exchanges (kInit's stores).
__global__ __launch_bounds__(TJ) void kWtoR(KParams k) {
  const int64_t n = k.nx * k.ny;
  for (int64_t idx = int64_t(blockIdx.x) * TJ + threadIdx.x; idx < n; idx += int64_t(gridDim.x) * TJ) {
    const int64_t li = idx / k.ny + 1, lj = idx % k.ny + 1;
    const double v = k.w[li * k.wpitch + lj];
    k.r[li * k.pitch + lj] = v;
    if (lj == 1 && k.has[DOWN]) k.send_dn[li - 1] = v;
    if (lj == k.ny && k.has[UP]) k.send_up[li - 1] = v;
  }
}
// … and after the exchange: recv_dn / recv_up → columns 0 / ny+1 of the r plane.
__global__ __launch_bounds__(TJ) void kUnpackR(KParams k) {
  for (int64_t li = int64_t(blockIdx.x) * TJ + threadIdx.x + 1; li <= k.nx; li += int64_t(gridDim.x) * TJ) {
    if (k.has[DOWN]) k.r[li * k.pitch] = k.recv_dn[li - 1];
    if (k.has[UP]) k.r[li * k.pitch + k.ny + 1] = k.recv_up[li - 1];
  }
}

// Gradient of w and its functionals (pe/fields.hpp gradient_field, the same
// expressions in the same order: the same bits).  `wp` is local (0, 0) of a
// plane holding w on the owned nodes and the neighbours' values on the ring
// (row stride `pitch`); ring values on the box boundary or outside the ellipse
// are loaded but never used.  Work: tiles of kGradCols columns × `trows` rows,
// tile t = (row band t / ctiles, column tile t % ctiles), dealt to the blocks
// round-robin.  A block marches down its tile with one column per lane (sj == 1
// stores coalesced), four rows per step: the rows above and below stay in
// registers, the rows' left / right neighbours are re-read through the cache —
// 8 B of w from memory and (STORE) 16 B written per node.  All indices 64-bit.
// Sums: block partials → arrive_last → the last block sums them in block order
// into st->res[0..2] = {Σ_D w, Σ_D (gx² + gy²), max_D (gx² + gy²)}.
constexpr int kGradCols = TJ, kGradU = 4;
__device__ __forceinline__ double grad_diff(bool in_lo, bool in_hi, double lo, double c, double hi, double h) {
  // (operands selected first: one subtraction and one division whichever case)
  const double a = in_hi ? hi : c, b = in_lo ? lo : c;
  const double den = in_lo && in_hi ? 2.0 * h : h;
  return in_lo || in_hi ? (a - b) / den : 0.0;
}
template <bool STORE>
__global__ __launch_bounds__(TJ) void kGradField(KParams k, const double* __restrict__ wp, int64_t pitch, int trows,
                                                 int64_t ctiles, int64_t ntiles, double* __restrict__ gx,
                                                 double* __restrict__ gy, int64_t si, int64_t sj, int64_t off_i,
                                                 int64_t off_j) {
  __shared__ double sm[8];
  __shared__ int sflag;
  DevState* st = k.st;
  double sw = 0.0, se = 0.0, mx = 0.0;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t band = t / ctiles, ct = t - band * ctiles;
    const int64_t lj0 = ct * kGradCols + threadIdx.x + 1;
    const bool live = lj0 <= k.ny;
    const int64_t lj = live ? lj0 : k.ny;  // (idle lanes of the last column tile load in range, store nothing)
    const int64_t gj = k.gj0 + lj;
    // cy·y² of columns j−1, j, j+1 (in_ellipse's own products); the box boundary is outside
    const double ym = k.A2 + (gj - 1) * k.h2, y0 = k.A2 + gj * k.h2, yp = k.A2 + (gj + 1) * k.h2;
    const double tym = k.cy * ym * ym, ty0 = k.cy * y0 * y0, typ = k.cy * yp * yp;
    const bool jm_ok = gj - 1 >= 1, jp_ok = gj + 1 <= k.N - 1;
    const int64_t li0 = band * trows + 1, li1 = min(k.nx, li0 + trows - 1);
    const double* col = wp + lj;
    double wm = col[(li0 - 1) * pitch], wc = col[li0 * pitch];
    for (int64_t li = li0; li <= li1; li += kGradU) {
      double dn[kGradU], dl[kGradU], dr[kGradU];
#pragma unroll
      for (int u = 0; u < kGradU; ++u) {  // (rows past the tile: clamped, loaded, unused)
        const int64_t q = min(li + u, li1);
        dn[u] = col[(q + 1) * pitch];
        dl[u] = col[q * pitch - 1];
        dr[u] = col[q * pitch + 1];
      }
#pragma unroll
      for (int u = 0; u < kGradU; ++u) {
        const int64_t q = li + u;
        if (q <= li1) {
          const int64_t gi = k.gi0 + q;
          const double xm = k.A1 + (gi - 1) * k.h1, x0 = k.A1 + gi * k.h1, xp = k.A1 + (gi + 1) * k.h1;
          const double txm = k.cx * xm * xm, tx0 = k.cx * x0 * x0, txp = k.cx * xp * xp;
          const bool in0 = tx0 + ty0 < 1.0;
          const bool in_im = gi - 1 >= 1 && txm + ty0 < 1.0, in_ip = gi + 1 <= k.M - 1 && txp + ty0 < 1.0;
          const bool in_jm = jm_ok && tx0 + tym < 1.0, in_jp = jp_ok && tx0 + typ < 1.0;
          double dx = 0.0, dy = 0.0;
          if (in0) {
            dx = grad_diff(in_im, in_ip, wm, wc, dn[u], k.h1);
            dy = grad_diff(in_jm, in_jp, dl[u], wc, dr[u], k.h2);
            if (live) {
              const double g2 = dx * dx + dy * dy;
              sw += wc;
              se += g2;
              mx = fmax(mx, g2);
            }
          }
          if (STORE && live) {
            const int64_t o = (off_i + q - 1) * si + (off_j + lj - 1) * sj;
            gx[o] = dx;
            gy[o] = dy;
          }
          wm = wc;
          wc = dn[u];
        }
      }
    }
  }
  double s[2] = {sw, se};
  double m[1] = {mx};
  block_reduce<2, false>(s, sm);
  __syncthreads();
  block_reduce<1, true>(m, sm);
  if (threadIdx.x == 0) {
    k.partial[3 * size_t(blockIdx.x)] = s[0];
    k.partial[3 * size_t(blockIdx.x) + 1] = s[1];
    k.partial[3 * size_t(blockIdx.x) + 2] = m[0];
  }
  if (arrive_last(&st->ticket[3], gridDim.x, &sflag)) {
    double a0 = 0.0, a1 = 0.0, m0 = 0.0;
    for (unsigned b = threadIdx.x; b < gridDim.x; b += TJ) {
      a0 += k.partial[3 * size_t(b)];
      a1 += k.partial[3 * size_t(b) + 1];
      m0 = fmax(m0, k.partial[3 * size_t(b) + 2]);
    }
    double s2[2] = {a0, a1};
    double mm[1] = {m0};
    block_reduce<2, false>(s2, sm);
    __syncthreads();
    block_reduce<1, true>(mm, sm);
    if (threadIdx.x == 0) {
      st->res[0] = s2[0];
      st->res[1] = s2[1];
      st->res[2] = mm[0];
      __hip_atomic_store(&st->ticket[3], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// The operator applied to a user field, and the residual field of an iterate
// (pe/fields.hpp apply_operator / residual_field, the same coefficients and
// expression tree).  `g` is element [0][0] of the caller's GLOBAL interior
// array (M−1) × (N−1), float64 or float32 (widened on load), element strides
// (si, sj) ≥ 0: no staging plane, no halo exchange — a block's ring values are
// its neighbours' entries of the same array, 0 on the box boundary.  Boundary
// neighbours are loaded at the clamped in-range index and selected to 0, so no
// load leaves the array.  kGradField's walk: tiles of kGradCols columns ×
// `trows` rows dealt round-robin, one column per lane, kApplyU rows per step;
// the rows above and below stay in registers, left / right neighbours are
// re-read through the cache — 8 B read and (STORE) 8 B written per node when
// sj == 1.  out = A v, or (RESID) B − A v with B = Bp (the user-rhs plane,
// dense nx × ny; null: F) inside the ellipse and 0 outside, written like
// kGatherW writes w.  Σ v·(A v) or (RESID) Σ out² over the owned nodes: block
// partials → arrive_last → the last block in block order → st->res[0].
// Reads tables only; of the state it writes res[0] and ticket[3].
constexpr int kApplyU = 4;
template <typename T>
__device__ __forceinline__ double field_at(const T* col, int64_t si, int64_t gi, int64_t gnx, bool col_ok) {
  const int64_t ci = gi < 1 ? 1 : (gi > gnx ? gnx : gi);  // (clamped: the load stays inside the array)
  const double v = double(col[(ci - 1) * si]);
  const bool ok = col_ok & (gi >= 1) & (gi <= gnx);  // (no short circuit: one select, the load above it stays unconditional)
  return ok ? v : 0.0;
}
// … of an owned row (1 ≤ gi ≤ M−1): only the column can be off the box
template <typename T>
__device__ __forceinline__ double field_in_row(const T* col, int64_t si, int64_t gi, bool col_ok) {
  const double v = double(col[(gi - 1) * si]);
  return col_ok ? v : 0.0;
}
// FIELD: c of the batch's rows from the reaction plane, loaded with the batch.
template <typename T, bool RESID, bool STORE, bool SHIFT = false, bool FIELD = false>
__global__ __launch_bounds__(TJ) void kApplyField(KParams k, const T* __restrict__ g, int64_t si, int64_t sj,
                                                  const double* __restrict__ Bp, int trows, int64_t ctiles,
                                                  int64_t ntiles, double* __restrict__ dst, int64_t dsi, int64_t dsj,
                                                  int64_t off_i, int64_t off_j) {
  __shared__ double sm[8];
  __shared__ int sflag;
  DevState* st = k.st;
  const int64_t gnx = int64_t(k.M) - 1, gny = int64_t(k.N) - 1;
  double acc = 0.0;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t band = t / ctiles, ct = t - band * ctiles;
    const int64_t lj0 = ct * kGradCols + threadIdx.x + 1;
    const bool live = lj0 <= k.ny;
    const int64_t lj = live ? lj0 : k.ny;  // (idle lanes of the last column tile load in range, store nothing)
    const int64_t gj = k.gj0 + lj;         // global node column, 1 .. N−1
    const bool jm_ok = gj - 1 >= 1, jp_ok = gj + 1 <= gny;
    // per-lane column pointers: this column, its left / right neighbour (clamped), the rhs plane, the destination
    const T* pc = g + (gj - 1) * sj;
    const T* pl = g + (jm_ok ? gj - 2 : 0) * sj;
    const T* pr = g + (jp_ok ? gj : gny - 1) * sj;
    const double y = k.A2 + gj * k.h2;
    const double ty = k.cy * y * y;  // (in_ellipse's own products: cx x² + cy y² < 1)
    const TV tv = tv_at(k, lj);
    const int64_t li0 = band * trows + 1, li1 = min(k.nx, li0 + trows - 1);
    // row li0 of this lane's column in the rhs plane (no plane: a table word is loaded instead and F selected,
    // so the load is unconditional and queues with the others) and in the destination
    const double* brow = Bp ? Bp + (li0 - 1) * k.ny + (lj - 1) : k.rowT;
    const int64_t bstep = Bp ? k.ny : 0;
    double* drow = STORE ? dst + (off_i + li0 - 1) * dsi + (off_j + lj - 1) * dsj : nullptr;
    double wm = field_at(pc, si, k.gi0 + li0 - 1, gnx, true), wc = field_at(pc, si, k.gi0 + li0, gnx, true);
    for (int64_t li = li0; li <= li1; li += kApplyU) {
      // a batch of kApplyU rows of loads, all issued before the first row is computed: the row below (dn), the
      // left / right neighbours (dl, dr), the rhs value (db).  Rows past the tile: clamped, loaded, unused.
      double dn[kApplyU], dl[kApplyU], dr[kApplyU], db[RESID ? kApplyU : 1], dc[FIELD ? kApplyU : 1] = {};
#pragma unroll
      for (int u = 0; u < kApplyU; ++u) {
        const int64_t r = min(li + u, li1), gi = k.gi0 + r;
        dn[u] = field_at(pc, si, gi + 1, gnx, true);
        dl[u] = field_in_row(pl, si, gi, jm_ok);
        dr[u] = field_in_row(pr, si, gi, jp_ok);
        if constexpr (RESID) db[u] = brow[(r - li0) * bstep];
        if constexpr (FIELD) dc[u] = k.creact[r * k.pitch + lj];
      }
#pragma unroll
      for (int u = 0; u < kApplyU; ++u) {
        const int64_t q = li + u;
        if (q <= li1) {
          const double cv = FIELD ? dc[u] : 0.0;
          const CS c = cset<true, SHIFT, FIELD>(k, k.rowcls + (q + 1) * 4, q, lj, tv, cv);
          const double Av = stencil<true, SHIFT, FIELD>(k, c, wm, wc, dn[u], dl[u], dr[u], cv);
          double o = Av;
          if constexpr (RESID) {
            const double x = k.A1 + (k.gi0 + q) * k.h1;
            const double B = k.cx * x * x + ty < 1.0 ? (Bp ? db[u] : k.F) : 0.0;
            o = B - Av;
          }
          if (live) acc += RESID ? o * o : wc * Av;
          if constexpr (STORE) {
            if (live) *drow = o;
            drow += dsi;
          }
          wm = wc;
          wc = dn[u];
        }
      }
    }
  }
  double s[1] = {acc};
  block_reduce<1, false>(s, sm);
  if (threadIdx.x == 0) k.partial[blockIdx.x] = s[0];
  if (arrive_last(&st->ticket[3], gridDim.x, &sflag)) {
    double a0 = 0.0;
    for (unsigned b = threadIdx.x; b < gridDim.x; b += TJ) a0 += k.partial[b];
    double s2[1] = {a0};
    block_reduce<1, false>(s2, sm);
    if (threadIdx.x == 0) {
      st->res[0] = s2[0];
      __hip_atomic_store(&st->ticket[3], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// p-plane of x[b] ← 0 over every allocated row and column (halos included):
// rows 1-hdep .. nx+hdep+2, columns -xorg .. poff-xorg-1.
__global__ __launch_bounds__(TJ) void kZeroP(KParams k, int b) {
  const int64_t h = k.hdep, rows = k.nx + 2 * h + 2, cols = k.poff;
  double* base = k.x[b] + k.poff - (h - 1) * k.pitch - k.xorg;
  for (int64_t idx = int64_t(blockIdx.x) * TJ + threadIdx.x; idx < rows * cols; idx += int64_t(gridDim.x) * TJ)
    base[(idx / cols) * k.pitch + idx % cols] = 0.0;
}

// Three-step restart (residual replacement): the solve goes on from the
// current iteration with a fresh recurrence — S_0 next (started = 0), no
// pending stop tests, and β = 0 for the iteration after k0 (fused3.hip).
__global__ void kRestart3(KParams k) {
  DevState* st = k.st;
  st->done = 0;
  st->status = 0;
  st->started = 0;
  st->late3 = 0;
  st->brk3 = 0;
  st->bad3 = 0;
  st->wpend = 0;
  st->fixj = 0;
  st->k0 = st->iter;
  st->sig = 0;  // (the host restarts its overlap epoch count with it)
}

// PE_FAULT_INJECT=drift@iter:K (test hook): w(li, lj) += v behind the
// recurrence's back — its r no longer is B − A w, which the end-of-solve
// residual check must see (and the three-step solve restart from).
__global__ void kSetStop(DevState* st, double thr, double nat0) {
  st->red_G[1] = thr;
  st->err[3] = nat0;
}
__global__ void kPokeW(KParams k, int64_t li, int64_t lj, double v) { k.w[li * k.wpitch + lj] += v; }

__global__ void kGroupReduce(double* const* bufs, int nranks, int n, int is_max) {
  const int i = threadIdx.x;
  if (i >= n) return;
  double acc = bufs[0][i];
  for (int r = 1; r < nranks; ++r) acc = is_max ? fmax(acc, bufs[r][i]) : acc + bufs[r][i];
  for (int r = 0; r < nranks; ++r) bufs[r][i] = acc;
}

// Test op: Ap = A p on owned nodes (p halo must be valid).
template <bool EXACT, bool SHIFT = false, bool FIELD = false>
__global__ void kApplyA(KParams k, const double* p, double* Ap) {
  const int64_t n = k.nx * k.ny;
  for (int64_t idx = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; idx < n;
       idx += int64_t(gridDim.x) * blockDim.x) {
    const int64_t li = idx / k.ny + 1, lj = idx % k.ny + 1;
    const int64_t c = li * k.pitch + lj;
    const CS cs = cset_mem<EXACT, SHIFT, FIELD>(k, li, lj);
    double cv = 0.0;
    if constexpr (FIELD) cv = k.creact[c];
    Ap[c] = stencil<EXACT, SHIFT, FIELD>(k, cs, p[c - k.pitch], p[c], p[c + k.pitch], p[c - 1], p[c + 1], cv);
  }
}

// Test op: a_ij, b_ij, D_ij through the class table (checks the classification).
template <bool SHIFT = false, bool FIELD = false>
__global__ void kCoef(KParams k, double* a, double* b, double* D) {
  const int64_t n = (k.nx + 2) * (k.ny + 2);
  for (int64_t idx = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; idx < n;
       idx += int64_t(gridDim.x) * blockDim.x) {
    const int64_t li = idx / (k.ny + 2), lj = idx % (k.ny + 2);
    const CS cs = cset_mem<true, SHIFT, FIELD>(k, li, lj);
    const int64_t c = li * k.pitch + lj;
    a[c] = cs.a0;
    b[c] = cs.b0;
    D[c] = cs.d;
  }
}

}  // namespace

int grid_blocks(const KParams& k) { return k.nblocks; }

// Test transport: a busy wait of `us` microseconds on the stream (one wave).
__global__ void kDelay(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
void launch_delay(double us, hipStream_t s) {
  int rate_khz = 100000;  // wall_clock64 runs at a fixed 100 MHz on CDNA
  (void)hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, 0);
  const long long ticks = (long long)(us * 1e-3 * double(rate_khz));
  hipLaunchKernelGGL(kDelay, dim3(1), dim3(64), 0, s, ticks);
}

int resident_blocks_classic(int variant, bool shift, bool field) {
  int n = 0, m = 0;
  if (field && variant == 1) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kF<true, false, true>, TJ, 0) != hipSuccess) n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&m, kG<true, false, true>, TJ, 0) != hipSuccess) m = 0;
  } else if (field) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kF<false, false, true>, TJ, 0) != hipSuccess) n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&m, kG<false, false, true>, TJ, 0) != hipSuccess) m = 0;
  } else if (shift && variant == 1) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kF<true, true>, TJ, 0) != hipSuccess) n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&m, kG<true, true>, TJ, 0) != hipSuccess) m = 0;
  } else if (shift) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kF<false, true>, TJ, 0) != hipSuccess) n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&m, kG<false, true>, TJ, 0) != hipSuccess) m = 0;
  } else if (variant == 1) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kF<true>, TJ, 0) != hipSuccess) n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&m, kG<true>, TJ, 0) != hipSuccess) m = 0;
  } else {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kF<false>, TJ, 0) != hipSuccess) n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&m, kG<false>, TJ, 0) != hipSuccess) m = 0;
  }
  return std::min(n, m);
}

static unsigned flat_blocks(const KParams& k) {
  const int64_t n = (k.nx + 2) * (k.ny + 2);
  int64_t b = (n + TJ - 1) / TJ;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return unsigned(b);
}

// Problem::shift ≠ 0 → the SHIFT instantiations; each wrapper decides here, once.
static bool shifted(const KParams& k) { return k.shift != 0.0; }
// Problem::reaction (the plane is set) → the FIELD instantiations, decided in the same places.
static bool fielded(const KParams& k) { return k.creact != nullptr; }

void launch_init(const KParams& k, int init_random, unsigned long long seed, double amp, int variant,
                 hipStream_t s) {
  if (fielded(k)) {
    if (variant == 1) hipLaunchKernelGGL((kInit<true, false, true>), dim3(flat_blocks(k)), dim3(TJ), 0, s, k, init_random, seed, amp);
    else hipLaunchKernelGGL((kInit<false, false, true>), dim3(flat_blocks(k)), dim3(TJ), 0, s, k, init_random, seed, amp);
    return;
  }
  if (shifted(k)) {
    if (variant == 1) hipLaunchKernelGGL((kInit<true, true>), dim3(flat_blocks(k)), dim3(TJ), 0, s, k, init_random, seed, amp);
    else hipLaunchKernelGGL((kInit<false, true>), dim3(flat_blocks(k)), dim3(TJ), 0, s, k, init_random, seed, amp);
    return;
  }
  if (variant == 1) hipLaunchKernelGGL(kInit<true>, dim3(flat_blocks(k)), dim3(TJ), 0, s, k, init_random, seed, amp);
  else hipLaunchKernelGGL(kInit<false>, dim3(flat_blocks(k)), dim3(TJ), 0, s, k, init_random, seed, amp);
}

void launch_init_field(const KParams& k, const double* rhs, const double* w0, int init_random,
                       unsigned long long seed, double amp, int variant, hipStream_t s) {
  if (fielded(k)) {
    if (variant == 1)
      hipLaunchKernelGGL((kInitField<true, false, true>), dim3(flat_blocks(k)), dim3(TJ), 0, s, k, rhs, w0, init_random, seed, amp);
    else
      hipLaunchKernelGGL((kInitField<false, false, true>), dim3(flat_blocks(k)), dim3(TJ), 0, s, k, rhs, w0, init_random, seed, amp);
    return;
  }
  if (shifted(k)) {
    if (variant == 1)
      hipLaunchKernelGGL((kInitField<true, true>), dim3(flat_blocks(k)), dim3(TJ), 0, s, k, rhs, w0, init_random, seed, amp);
    else
      hipLaunchKernelGGL((kInitField<false, true>), dim3(flat_blocks(k)), dim3(TJ), 0, s, k, rhs, w0, init_random, seed, amp);
    return;
  }
  if (variant == 1)
    hipLaunchKernelGGL(kInitField<true>, dim3(flat_blocks(k)), dim3(TJ), 0, s, k, rhs, w0, init_random, seed, amp);
  else
    hipLaunchKernelGGL(kInitField<false>, dim3(flat_blocks(k)), dim3(TJ), 0, s, k, rhs, w0, init_random, seed, amp);
}

void launch_F(const KParams& k, int par, int variant, hipStream_t s) {
  if (fielded(k)) {
    if (variant == 1) hipLaunchKernelGGL((kF<true, false, true>), dim3(k.nblocks), dim3(TJ), 0, s, k, par);
    else hipLaunchKernelGGL((kF<false, false, true>), dim3(k.nblocks), dim3(TJ), 0, s, k, par);
    return;
  }
  if (shifted(k)) {
    if (variant == 1) hipLaunchKernelGGL((kF<true, true>), dim3(k.nblocks), dim3(TJ), 0, s, k, par);
    else hipLaunchKernelGGL((kF<false, true>), dim3(k.nblocks), dim3(TJ), 0, s, k, par);
    return;
  }
  if (variant == 1) hipLaunchKernelGGL(kF<true>, dim3(k.nblocks), dim3(TJ), 0, s, k, par);
  else hipLaunchKernelGGL(kF<false>, dim3(k.nblocks), dim3(TJ), 0, s, k, par);
}

void launch_G(const KParams& k, int par, int variant, hipStream_t s) {
  if (fielded(k)) {
    if (variant == 1) hipLaunchKernelGGL((kG<true, false, true>), dim3(k.nblocks), dim3(TJ), 0, s, k, par);
    else hipLaunchKernelGGL((kG<false, false, true>), dim3(k.nblocks), dim3(TJ), 0, s, k, par);
    return;
  }
  if (shifted(k)) {
    if (variant == 1) hipLaunchKernelGGL((kG<true, true>), dim3(k.nblocks), dim3(TJ), 0, s, k, par);
    else hipLaunchKernelGGL((kG<false, true>), dim3(k.nblocks), dim3(TJ), 0, s, k, par);
    return;
  }
  if (variant == 1) hipLaunchKernelGGL(kG<true>, dim3(k.nblocks), dim3(TJ), 0, s, k, par);
  else hipLaunchKernelGGL(kG<false>, dim3(k.nblocks), dim3(TJ), 0, s, k, par);
}

// Word copy by a kernel (host-mapped pinned memory on either side): the
// solver's set-up uploads and per-chunk state reads, so that no hipMemcpy
// runs in T_solver — a fresh process's first hipMemcpy costs 17-170 ms of
// runtime initialisation (profiles/r2_ctor.txt), a kernel 0.5 ms.
__global__ __launch_bounds__(256) void kCopyWords(const unsigned* __restrict__ src, unsigned* __restrict__ dst,
                                                  int64_t n, int to_host) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    dst[i] = src[i];
  if (to_host) __threadfence_system();
}

void launch_copy_words(void* dst, const void* src, size_t bytes, bool to_host, hipStream_t s) {
  const int64_t n = int64_t(bytes / 4);
  if (n == 0) return;
  const unsigned g = unsigned(std::min<int64_t>(1024, (n + 255) / 256));
  hipLaunchKernelGGL(kCopyWords, dim3(g), dim3(256), 0, s, static_cast<const unsigned*>(src),
                     static_cast<unsigned*>(dst), n, to_host ? 1 : 0);
}

static unsigned copy_blocks(int64_t n) { return unsigned(std::max<int64_t>(1, std::min<int64_t>(4096, (n + 255) / 256))); }

void launch_slice_field(const void* g, bool f32, int64_t si, int64_t sj, int64_t gnx, int64_t gny, int64_t i0,
                        int64_t j0, int64_t nx, int64_t ny, int ring, double* out, hipStream_t s) {
  const int64_t rows = nx + 2 * ring, cols = ny + 2 * ring;
  const dim3 grid(copy_blocks(rows * cols)), block(256);
  const float* gf = static_cast<const float*>(g);
  const double* gd = static_cast<const double*>(g);
  if (f32 && ring) hipLaunchKernelGGL((kSliceField<float, 1>), grid, block, 0, s, gf, si, sj, gnx, gny, i0, j0, rows, cols, out);
  else if (f32) hipLaunchKernelGGL((kSliceField<float, 0>), grid, block, 0, s, gf, si, sj, gnx, gny, i0, j0, rows, cols, out);
  else if (ring) hipLaunchKernelGGL((kSliceField<double, 1>), grid, block, 0, s, gd, si, sj, gnx, gny, i0, j0, rows, cols, out);
  else hipLaunchKernelGGL((kSliceField<double, 0>), grid, block, 0, s, gd, si, sj, gnx, gny, i0, j0, rows, cols, out);
}

void launch_ring_to_pitched(const double* ring, int64_t nx, int64_t ny, double* dst, int64_t pitch, hipStream_t s) {
  const int64_t rows = nx + 2, cols = ny + 2;
  hipLaunchKernelGGL(kRingToPitched, dim3(copy_blocks(rows * cols)), dim3(256), 0, s, ring, rows, cols, dst, pitch);
}

void launch_gather_w(const KParams& k, double* dst, int64_t si, int64_t sj, int64_t off_i, int64_t off_j,
                     hipStream_t s) {
  hipLaunchKernelGGL(kGatherW, dim3(copy_blocks(k.nx * k.ny)), dim3(256), 0, s, k.w, k.wpitch, k.nx, k.ny, dst, si, sj,
                     off_i, off_j);
}

void launch_error(const KParams& k, hipStream_t s, const double* exact) {
  if (exact) hipLaunchKernelGGL(kErrorField, dim3(flat_blocks(k)), dim3(TJ), 0, s, k, exact);
  else hipLaunchKernelGGL(kError, dim3(flat_blocks(k)), dim3(TJ), 0, s, k);
}

void launch_resid(const KParams& k, int bw, bool with_r, bool store, hipStream_t s, const double* rhs) {
  if (rhs) hipLaunchKernelGGL(kResidField, dim3(flat_blocks(k)), dim3(TJ), 0, s, k, bw, with_r ? 1 : 0, store ? 1 : 0, rhs);
  else hipLaunchKernelGGL(kResid, dim3(flat_blocks(k)), dim3(TJ), 0, s, k, bw, with_r ? 1 : 0, store ? 1 : 0);
}
void launch_w_to_p(const KParams& k, int b, hipStream_t s) {
  hipLaunchKernelGGL(kWtoP, dim3(flat_blocks(k)), dim3(TJ), 0, s, k, b);
}
void launch_w_to_r(const KParams& k, hipStream_t s) {
  hipLaunchKernelGGL(kWtoR, dim3(flat_blocks(k)), dim3(TJ), 0, s, k);
}
void launch_unpack_r(const KParams& k, hipStream_t s) {
  if (!k.has[DOWN] && !k.has[UP]) return;
  const unsigned g = unsigned(std::max<int64_t>(1, std::min<int64_t>(1024, (k.nx + TJ - 1) / TJ)));
  hipLaunchKernelGGL(kUnpackR, dim3(g), dim3(TJ), 0, s, k);
}
void launch_grad_field(const KParams& k, const double* plane, int64_t pitch, double* gx, double* gy, int64_t si,
                       int64_t sj, int64_t off_i, int64_t off_j, hipStream_t s) {
  // Rows per tile: enough tiles to fill the device (≈ 2048) where the block
  // has them, between 8 rows (small blocks still make several tiles) and 64
  // (the two ring rows a tile re-reads stay ≈ 3 % of its loads).  At most 4096
  // blocks (k.partial holds 3 doubles for each); larger tile counts wrap.
  const int64_t ctiles = (k.ny + kGradCols - 1) / kGradCols;
  const int64_t bands = std::max<int64_t>(1, 2048 / ctiles);
  const int trows = int(std::max<int64_t>(8, std::min<int64_t>(64, (k.nx + bands - 1) / bands)));
  const int64_t ntiles = ctiles * ((k.nx + trows - 1) / trows);
  const dim3 grid(unsigned(std::min<int64_t>(ntiles, 4096))), block(TJ);
  if (gx && gy)
    hipLaunchKernelGGL(kGradField<true>, grid, block, 0, s, k, plane, pitch, trows, ctiles, ntiles, gx, gy, si, sj,
                       off_i, off_j);
  else
    hipLaunchKernelGGL(kGradField<false>, grid, block, 0, s, k, plane, pitch, trows, ctiles, ntiles,
                       static_cast<double*>(nullptr), static_cast<double*>(nullptr), int64_t(0), int64_t(0), int64_t(0),
                       int64_t(0));
}
namespace {
template <typename T, bool RESID, bool SHIFT, bool FIELD = false>
void apply_field_launch(const KParams& k, const T* g, int64_t si, int64_t sj, const double* rhs, double* dst,
                        int64_t dsi, int64_t dsj, int64_t off_i, int64_t off_j, hipStream_t s) {
  // launch_grad_field's tiling: ≈ 2048 tiles where the block has them, 8 .. 64 rows each, ≤ 4096 blocks
  const int64_t ctiles = (k.ny + kGradCols - 1) / kGradCols;
  const int64_t bands = std::max<int64_t>(1, 2048 / ctiles);
  const int trows = int(std::max<int64_t>(8, std::min<int64_t>(64, (k.nx + bands - 1) / bands)));
  const int64_t ntiles = ctiles * ((k.nx + trows - 1) / trows);
  const dim3 grid(unsigned(std::min<int64_t>(ntiles, 4096))), block(TJ);
  if (dst)
    hipLaunchKernelGGL((kApplyField<T, RESID, true, SHIFT, FIELD>), grid, block, 0, s, k, g, si, sj, rhs, trows, ctiles, ntiles, dst,
                       dsi, dsj, off_i, off_j);
  else
    hipLaunchKernelGGL((kApplyField<T, RESID, false, SHIFT, FIELD>), grid, block, 0, s, k, g, si, sj, rhs, trows, ctiles, ntiles,
                       static_cast<double*>(nullptr), int64_t(0), int64_t(0), int64_t(0), int64_t(0));
}
}  // namespace
void launch_apply_field(const KParams& k, const void* g, bool f32, int64_t si, int64_t sj, bool resid,
                        const double* rhs, double* dst, int64_t dsi, int64_t dsj, int64_t off_i, int64_t off_j,
                        hipStream_t s) {
  const float* gf = static_cast<const float*>(g);
  const double* gd = static_cast<const double*>(g);
  if (fielded(k)) {
    if (f32 && resid) apply_field_launch<float, true, false, true>(k, gf, si, sj, rhs, dst, dsi, dsj, off_i, off_j, s);
    else if (f32) apply_field_launch<float, false, false, true>(k, gf, si, sj, rhs, dst, dsi, dsj, off_i, off_j, s);
    else if (resid) apply_field_launch<double, true, false, true>(k, gd, si, sj, rhs, dst, dsi, dsj, off_i, off_j, s);
    else apply_field_launch<double, false, false, true>(k, gd, si, sj, rhs, dst, dsi, dsj, off_i, off_j, s);
    return;
  }
  if (shifted(k)) {
    if (f32 && resid) apply_field_launch<float, true, true>(k, gf, si, sj, rhs, dst, dsi, dsj, off_i, off_j, s);
    else if (f32) apply_field_launch<float, false, true>(k, gf, si, sj, rhs, dst, dsi, dsj, off_i, off_j, s);
    else if (resid) apply_field_launch<double, true, true>(k, gd, si, sj, rhs, dst, dsi, dsj, off_i, off_j, s);
    else apply_field_launch<double, false, true>(k, gd, si, sj, rhs, dst, dsi, dsj, off_i, off_j, s);
    return;
  }
  if (f32 && resid) apply_field_launch<float, true, false>(k, gf, si, sj, rhs, dst, dsi, dsj, off_i, off_j, s);
  else if (f32) apply_field_launch<float, false, false>(k, gf, si, sj, rhs, dst, dsi, dsj, off_i, off_j, s);
  else if (resid) apply_field_launch<double, true, false>(k, gd, si, sj, rhs, dst, dsi, dsj, off_i, off_j, s);
  else apply_field_launch<double, false, false>(k, gd, si, sj, rhs, dst, dsi, dsj, off_i, off_j, s);
}
void launch_zero_p(const KParams& k, int b, hipStream_t s) {
  hipLaunchKernelGGL(kZeroP, dim3(flat_blocks(k)), dim3(TJ), 0, s, k, b);
}
void launch_restart3(const KParams& k, hipStream_t s) { hipLaunchKernelGGL(kRestart3, dim3(1), dim3(1), 0, s, k); }
void launch_set_stop(const KParams& k, double thr, double nat0, hipStream_t s) {
  hipLaunchKernelGGL(kSetStop, dim3(1), dim3(1), 0, s, k.st, thr, nat0);
}
void launch_poke_w(const KParams& k, int64_t li, int64_t lj, double v, hipStream_t s) {
  hipLaunchKernelGGL(kPokeW, dim3(1), dim3(1), 0, s, k, li, lj, v);
}

void launch_group_reduce(double* const* bufs, int nranks, int n, int is_max, hipStream_t s) {
  hipLaunchKernelGGL(kGroupReduce, dim3(1), dim3(64), 0, s, bufs, nranks, n, is_max);
}

void launch_apply_A(const KParams& k, const double* p, double* Ap, hipStream_t s) {
  if (fielded(k)) hipLaunchKernelGGL((kApplyA<false, false, true>), dim3(flat_blocks(k)), dim3(TJ), 0, s, k, p, Ap);
  else if (shifted(k)) hipLaunchKernelGGL((kApplyA<false, true>), dim3(flat_blocks(k)), dim3(TJ), 0, s, k, p, Ap);
  else hipLaunchKernelGGL(kApplyA<false>, dim3(flat_blocks(k)), dim3(TJ), 0, s, k, p, Ap);
}

void launch_coef(const KParams& k, double* a, double* b, double* D, hipStream_t s) {
  if (fielded(k)) hipLaunchKernelGGL((kCoef<false, true>), dim3(flat_blocks(k)), dim3(TJ), 0, s, k, a, b, D);
  else if (shifted(k)) hipLaunchKernelGGL(kCoef<true>, dim3(flat_blocks(k)), dim3(TJ), 0, s, k, a, b, D);
  else hipLaunchKernelGGL(kCoef<false>, dim3(flat_blocks(k)), dim3(TJ), 0, s, k, a, b, D);
}

}  // namespace dev
}  // namespace pe
