// pfsgnn_sl_loss.hip -- the training objective (train.py:29-80) on a sliced
// general batch (include/pfsgnn.h pfsgnn_sliced_t; layout: pfsgnn_sliced.hip).
//
// The reference indexes edges by position, which only means something on the
// complete fiber-major graph; here every edge is indexed by edge_index:
// T_e = class_info[tgt_e, 0], n'_c sums over tgt_e = c, fiber_time_f over
// src_e = f, the per-class variance runs over the deg(c) edges of the class
// (unbiased; 0 when deg(c) < 2, where torch.var would give NaN), and softfloor's
// uniform of edge e is pf_uniform(key, e) with e the CALLER's edge position --
// the counter of the dense kernel, independent of the sliced layout.
//
// Grid: the sliced edge kernels' (block = 4 waves = 4 slices = 64 fibers of one
// graph, KS step splits per slice).  The work per edge is scalar (decoder_e's
// F x F layer on the VALU, as k_loss_fwd), so a lane owns an EDGE, not a
// channel group: lane (q = lane >> 4, j = lane & 15) takes fiber j of the slice
// at step k0 + 4 i + q, i.e. position pb + 16 k0 + 64 i + lane -- a channel row,
// the class byte and the caller's edge id are each one coalesced access per
// four steps.  A lane's fiber is fixed, so fiber sums are thread-local and the
// four q groups are added in fixed order.  Class statistics (sum galaxies,
// count, mean tt, M2 tt) go to wave-private LDS rows: a row of 16 lanes whose
// edges share one class (complete-like slices) is reduced across lanes first
// and merged by one lane (Chan), rows in fixed order; otherwise the lanes
// update their classes' rows one edge at a time (Welford) in owner-slot rounds,
// as acc_add of pfsgnn_sliced.hip -- no float atomics, one wave's updates of a
// row in a fixed order.  The 4 waves merge in fixed order into the
// [G][NFG * KS][NC][4] partials k_loss_class_reduce finishes in double.
#include "pfsgnn_loss_core.h"
#include "pfsgnn_mfma.h"
#include "../../include/pfsgnn.h"

namespace {

using pfm::SlGeo;
constexpr int MAXC = pfm::SL_MAX_NC;
// a class row: sum galaxies, count, mean tt, M2 tt (+ 1 float: the rows of
// different classes spread over the LDS banks)
constexpr int CST = 5;

// sum over the lane's row of 16 lanes, in every lane of the row (fixed DPP tree)
__device__ __forceinline__ float row_sum16(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false));
  return v;
}

// (count n, mean m, M2 q, sum galaxies s) merged into a class row [Chan et al.]
__device__ __forceinline__ void row_merge(float* a, float s, float n, float m, float q) {
  const float ca = a[1], tot = ca + n;
  const float d = m - a[2];
  a[0] += s;
  a[1] = tot;
  a[2] = fmaf(d, n / tot, a[2]);
  a[3] += q + d * d * (ca * n / tot);
}

// the iteration's 64 edges into their classes' rows of the wave's table
__device__ __forceinline__ void class_add(float* wrow, int* own, int cl, bool ev, int lane,
                                          float gal, float tt) {
  const uint64_t vm = __ballot(ev);
  if (vm == 0) return;
  // the class of the first valid edge of the lane's row of 16
  const uint32_t rowm = (uint32_t)(vm >> (lane & 48)) & 0xFFFFu;
  const int first = (lane & 48) + (rowm ? __builtin_ctz(rowm) : 0);
  const int c0 = __shfl(cl, first);
  if (__ballot(ev && cl != c0) == 0) {
    // every row's edges share one class: reduce across the row, one lane merges
    const float n = (float)__builtin_popcount(rowm);
    const float s = row_sum16(ev ? gal : 0.f);
    const float m = n > 0.f ? row_sum16(ev ? tt : 0.f) / n : 0.f;
    const float d = ev ? tt - m : 0.f;
    const float q = row_sum16(d * d);
#pragma unroll
    for (int r = 0; r < 4; ++r) {   // (two rows may hold the same class: fixed order)
      if (lane == 16 * r && n > 0.f) row_merge(wrow + c0 * CST, s, n, m, q);
      wave_lds_sync();
    }
    return;
  }
  // owner-slot rounds: each pending lane writes its index to its class's slot;
  // the lane that reads its own index back updates the row, the others wait
  float* a = wrow + cl * CST;
  bool pend = ev;
  while (__ballot(pend) != 0) {
    if (pend) own[cl] = lane;
    wave_lds_sync();
    const bool win = pend && own[cl] == lane;
    if (win) {   // Welford
      const float c = a[1] + 1.f;
      const float d = tt - a[2];
      const float m = a[2] + d / c;
      a[0] += gal;
      a[1] = c;
      a[2] = m;
      a[3] = fmaf(d, tt - m, a[3]);
    }
    wave_lds_sync();
    pend = pend && !win;
  }
}

template <int F>
__global__ __launch_bounds__(256) void ksl_loss_fwd(
    EdgeGeo geo, SlGeo sl, const int* __restrict__ pos_user, const float* __restrict__ y,
    const float* __restrict__ sc, const float* __restrict__ sh, const float* __restrict__ Wd1,
    const float* __restrict__ bd1, const float* __restrict__ Wd2, const float* __restrict__ bd2,
    const float* __restrict__ ci, float scale, SoftFloor sf0,
    const SoftFloor* __restrict__ sf_dev, float noiselevel, uint64_t key0,
    const unsigned long long* __restrict__ seed_dev, float* __restrict__ fiber_time,
    float* __restrict__ tt_out, float* __restrict__ part) {
  SLL_PROLOGUE
  const uint64_t key = seed_dev ? pf_noise_key(*seed_dev) : key0;
  const SoftFloor sf = sf_dev ? *sf_dev : sf0;   // wave-uniform: scalar loads
  __shared__ float crow[4][MAXC * CST];
  __shared__ int own[4][MAXC];
  __shared__ __attribute__((aligned(16))) DecW<F> dw;
  dw.load(Wd1, bd1, Wd2, bd2);
  for (int i = t; i < 4 * MAXC * CST; i += PF_BLOCK) (&crow[0][0])[i] = 0.f;
  __syncthreads();
  float ft = 0.f;
  SLL_LOAD_DECL(F)
  SlEdge<F> cur = load(0);
  for (int i = 0; i < nit; ++i) {
    const SlEdge<F> nxt = load(i + 1);
    SLL_STEP(cur)
    float x[F];
#pragma unroll
    for (int k = 0; k < F; ++k) x[k] = sc ? fmaf(cur.y[k], sc[k], sh[k]) : cur.y[k];
    const float noise = noiselevel * (pf_uniform(key, (uint64_t)(ev ? cur.pos : 0)) - 0.5f);
    EdgeLoss<F> L;
    const float* dwp = dec_base(dw);
    L.run(x, dwp, dwp + F * F, dwp + F * F + F, dwp + F * F + 2 * F, scale, ci[cn], noise, sf);
    const float tt = ev ? L.tt : 0.f;
    ft += tt;
    if (tt_out && ev) tt_out[cur.pos] = L.tt;
    class_add(crow[wave], own[wave], cl, ev, lane, L.gal, L.tt);
    cur = nxt;
  }
  // fiber time: the four step groups of a fiber in fixed order, KS-partial per
  // global fiber (every fiber of the batch is one lane of one slice: 0 for a
  // fiber without edges)
  {
    const float f0 = __shfl(ft, j16), f1 = __shfl(ft, j16 + 16);
    const float f2 = __shfl(ft, j16 + 32), f3 = __shfl(ft, j16 + 48);
    if (q4 == 0 && fib >= 0) fiber_time[(size_t)ks * NS + fib] = ((f0 + f1) + f2) + f3;
  }
  // class partials: the 4 waves' rows merged in fixed order
  __syncthreads();
  const long long colbase = ((long long)grp * geo.KS + ks) * NC;
  for (int c = t; c < NC; c += PF_BLOCK) {
    double P = 0, C = 0, M = 0, Q = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float* a = crow[w] + c * CST;
      const double n = a[1];
      if (n > 0) {
        const double tot = C + n, d = (double)a[2] - M;
        M += d * (n / tot);
        Q += (double)a[3] + d * d * (C * n / tot);
        C = tot;
        P += a[0];
      }
    }
    float* o = part + (colbase + c) * 4;
    o[0] = (float)P; o[1] = (float)C; o[2] = (float)M; o[3] = (float)Q;
  }
}

__global__ void ksl_fiber_partial_sum(const float* __restrict__ part, int KS, long long len,
                                      float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= len) return;
  float s = 0.f;
  for (int k = 0; k < KS; ++k) s += part[(size_t)k * len + idx];
  out[idx] = s;
}

// k_loss_bwd on slices: the forward recomputed per edge, g_tt = Gf[fiber] +
// Gv[c] (tt - tmean[c]); gxe [F][EP] in slot order, every position of the
// block's steps written once (0 at padding: the sliced edge kernels rely on it)
template <int F>
__global__ __launch_bounds__(256) void ksl_loss_bwd(
    EdgeGeo geo, SlGeo sl, const int* __restrict__ pos_user, const float* __restrict__ y,
    const float* __restrict__ sc, const float* __restrict__ sh, const float* __restrict__ Wd1,
    const float* __restrict__ bd1, const float* __restrict__ Wd2, const float* __restrict__ bd2,
    const float* __restrict__ ci, float scale, SoftFloor sf0,
    const SoftFloor* __restrict__ sf_dev, float noiselevel, uint64_t key0,
    const unsigned long long* __restrict__ seed_dev, const float* __restrict__ Gn,
    const float* __restrict__ Gf, const float* __restrict__ Gv, const float* __restrict__ tmean,
    const float* __restrict__ gscale, float* __restrict__ gxe, float* __restrict__ partW,
    float* __restrict__ partV) {
  using WG = WGrad<F, F + 1>;  // g_zd (x) [x, 1] -> dWd1 | dbd1
  SLL_PROLOGUE
  const uint64_t key = seed_dev ? pf_noise_key(*seed_dev) : key0;
  const SoftFloor sf = sf_dev ? *sf_dev : sf0;   // wave-uniform: scalar loads
  constexpr int LDS_N = (4 * WG::LDS_FLOATS > 4 * F * (F + 1)) ? 4 * WG::LDS_FLOATS
                                                                : 4 * F * (F + 1);
  __shared__ float lds[LDS_N + 4 * (F + 1)];
  __shared__ __attribute__((aligned(16))) DecW<F> dw;
  dw.load(Wd1, bd1, Wd2, bd2);
  __syncthreads();
  float* region = lds + wave * WG::LDS_FLOATS;
  WG wg;
  wg.zero();
  float acc[F + 1];
#pragma unroll
  for (int j = 0; j <= F; ++j) acc[j] = 0.f;
  const float gs = gscale ? gscale[0] : 1.f;
  const float Gf_f = fib >= 0 ? Gf[fib] : 0.f;
  SLL_LOAD_DECL(F)
  SlEdge<F> cur = load(0);
  for (int i = 0; i < nit; ++i) {
    const SlEdge<F> nxt = load(i + 1);
    SLL_STEP(cur)
    const float Ti = ci[cn], Gn_c = Gn[cn], Gv_c = Gv[cn], tm_c = tmean[cn];
    float x[F + 1], xf[F];
#pragma unroll
    for (int k = 0; k < F; ++k) xf[k] = x[k] = sc ? fmaf(cur.y[k], sc[k], sh[k]) : cur.y[k];
    x[F] = 1.f;
    const float noise = noiselevel * (pf_uniform(key, (uint64_t)(ev ? cur.pos : 0)) - 0.5f);
    EdgeLoss<F> L;
    const float* dwp = dec_base(dw);
    L.run(xf, dwp, dwp + F * F, dwp + F * F + F, dwp + F * F + 2 * F, scale, Ti, noise, sf);
    const float g_tt = Gf_f + Gv_c * (L.tt - tm_c);
    const float g_gal = Gn_c + Ti * g_tt;
    const float mask = L.graw > 0.f ? 1.f : (L.graw == 0.f ? 0.5f : 0.f);
    const float cth = L.cth;
    const float dsf = 1.f + 2.f * (sf.r * cth - sf.r * sf.r) / (1.f - 2.f * sf.r * cth + sf.r * sf.r);
#if LOSS_FAST
    const float g_time = g_gal * mask * dsf * L.invTi;
#else
    const float g_time = g_gal * mask * dsf / Ti;
#endif
    const float sig = L.pred > 20.f ? 1.f : 1.f / (1.f + expf(-L.pred));
    const float g_pred = ev ? gs * g_time * scale * sig : 0.f;
    float gz[F];
#pragma unroll
    for (int j = 0; j < F; ++j) {
      acc[j] = fmaf(g_pred, L.ad[j], acc[j]);
      gz[j] = dwp[F * F + F + j] * g_pred * dlrelu(L.zd[j]);
    }
    acc[F] += g_pred;
    if (cur.in) {
      const long long p = p0 + 64ll * i;
#pragma unroll
      for (int k = 0; k < F; ++k) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < F; ++j) s = fmaf(dwp[j * F + k], gz[j], s);
        gxe[(long long)k * EP + p] = ev ? s : 0.f;
      }
    }
    wg.stage(region, gz, x, lane);
    wave_lds_sync();
    wg.accum(region, lane);
    wave_lds_sync();
    cur = nxt;
  }
  wg.block_partial(lds, partW + (size_t)bx * F * (F + 1));
  block_sum<F + 1>(acc, lds + LDS_N);
  if (t <= F) {
    float val = 0.f;
#pragma unroll
    for (int i = 0; i <= F; ++i) val = (i == t) ? acc[i] : val;
    partV[(size_t)bx * (F + 1) + t] = val;
  }
}

// ------------------------------------------------------------ host side
SlGeo sl_of(const pfsgnn_sliced_t& s) {
  return SlGeo{s.fib, s.base, s.len, s.cls, s.pco, s.EP, s.E, s.maxdeg};
}

// refuses, before any launch: bad dims, Fdim outside 8 / 10 / 16, a broken
// layout, an edge path without sliced kernels, NC above pfsgnn_sliced_max_nc
int check_sl(const char* where, const pfsgnn_sliced_t* sl, int G, int NF, int NC, int F) {
  if (G <= 0 || NF <= 1 || NC <= 0) return pf::fail(where, "need G > 0, NF > 1, NC > 0");
  if (F != 8 && F != 10 && F != 16) return pf::fail(where, "unsupported Fdim (8, 10, 16)");
  if (!sl || !sl->fib || !sl->base || !sl->len || !sl->cls || sl->EP <= 0 || sl->E <= 0 ||
      sl->EP < sl->E)
    return pf::fail(where, "bad sliced layout");
  if (sl->EP * F * 4 >= (1ll << 32)) return pf::fail(where, "edge tensor exceeds 4 GiB (split the batch)");
  int m = 0;
  if (int rc = pfsgnn_sliced_max_nc(F, &m)) return rc;
  if (m <= 0) return pf::fail(where, "sliced layout: the current edge path has no sliced kernels");
  if (NC > m || NC > MAXC)
    return pf::fail(where, "sliced layout: too many classes per graph (pfsgnn_sliced_max_nc)");
  return 0;
}

}  // namespace

// the sliced forms of the loss ops: pfsgnn_loss_fwd / pfsgnn_loss_bwd
// (pfsgnn_loss.hip) with a->sl set, sl and pos_user paired there
int pf_sl_loss_fwd(const pfsgnn_loss_args& a, void* ws, size_t ws_bytes, void* stream) {
  const char* where = "pfsgnn_loss_fwd";
  const int G = a.G, NF = a.NF, NC = a.NC, F = a.F;
  if (int rc = check_sl(where, a.sl, G, NF, NC, F)) return rc;
  PF_REQUIRE(a.pos_user && a.y && a.Wd1 && a.bd1 && a.Wd2 && a.bd2 && a.ci && a.n_prime &&
                 a.fiber_time && a.tmean && a.tvar,
             where, "null");
  const SlGeo sg = sl_of(*a.sl);
  const EdgeGeo geo = pfm::sl_geo(G, NF, NC, sg);
  const int bpg = geo.NFG * geo.KS;   // class-partial rows per graph
  LossWs w{reinterpret_cast<char*>(ws), ws_bytes};
  float* part = w.take((size_t)G * bpg * NC * 4);
  float* ftp = geo.KS == 1 ? a.fiber_time : w.take((size_t)geo.KS * geo.NS);
  PF_REQUIRE(part && ftp, where, "workspace too small");
  hipStream_t st = as_stream(stream);
  const SoftFloor sf = make_softfloor(a.sharpness);
  const SoftFloor* sfd = reinterpret_cast<const SoftFloor*>(a.sf_dev);
  const uint64_t key = pf_noise_key((uint64_t)a.seed);
  { pf::Timer tm_("loss_fwd", st);
  LOSS_DISPATCH_F(F, hipLaunchKernelGGL(ksl_loss_fwd<FF>, dim3(geo.nblocks), dim3(256), 0, st, geo,
                                        sg, a.pos_user, a.y, a.sc, a.sh, a.Wd1, a.bd1, a.Wd2, a.bd2,
                                        a.ci, a.scale, sf, sfd, a.noiselevel, key, a.seed_dev, ftp,
                                        a.tt, part));
  tm_.end(); }
  if (geo.KS > 1)
    hipLaunchKernelGGL(ksl_fiber_partial_sum, dim3((unsigned)((geo.NS + 255) / 256)), dim3(256), 0,
                       st, ftp, geo.KS, geo.NS, a.fiber_time);
  hipLaunchKernelGGL(k_loss_class_reduce<true>, dim3((G * NC + 3) / 4), dim3(256), 0, st, part, G,
                     bpg, NC, NF, a.n_prime, a.tmean, a.tvar);
  return pf::check_launch(where);
}

int pf_sl_loss_bwd(const pfsgnn_loss_args& a, void* ws, size_t ws_bytes, void* stream) {
  const char* where = "pfsgnn_loss_bwd";
  const int G = a.G, NF = a.NF, NC = a.NC, F = a.F;
  if (int rc = check_sl(where, a.sl, G, NF, NC, F)) return rc;
  PF_REQUIRE(a.pos_user && a.y && a.Wd1 && a.bd1 && a.Wd2 && a.bd2 && a.ci && a.Gn && a.Gf &&
                 a.Gv && a.tmean && a.dWd1 && a.dbd1 && a.dWd2 && a.dbd2 && a.gxe,
             where, "null");
  const SlGeo sg = sl_of(*a.sl);
  const EdgeGeo geo = pfm::sl_geo(G, NF, NC, sg);
  const size_t nb = geo.nblocks;
  LossWs w{reinterpret_cast<char*>(ws), ws_bytes};
  float* pW = w.take(nb * F * (F + 1));
  float* pV = w.take(nb * (F + 1));
  PF_REQUIRE(pW && pV, where, "workspace too small");
  hipStream_t st = as_stream(stream);
  const SoftFloor sf = make_softfloor(a.sharpness);
  const SoftFloor* sfd = reinterpret_cast<const SoftFloor*>(a.sf_dev);
  const uint64_t key = pf_noise_key((uint64_t)a.seed);
  { pf::Timer tm_("loss_bwd", st);
  LOSS_DISPATCH_F(F, hipLaunchKernelGGL(ksl_loss_bwd<FF>, dim3(geo.nblocks), dim3(256), 0, st, geo,
                                        sg, a.pos_user, a.y, a.sc, a.sh, a.Wd1, a.bd1, a.Wd2, a.bd2,
                                        a.ci, a.scale, sf, sfd, a.noiselevel, key, a.seed_dev, a.Gn,
                                        a.Gf, a.Gv, a.tmean, a.gscale, a.gxe, pW, pV));
  tm_.end(); }
  loss_bwd_reduce(a, pW, pV, nb, st);
  return pf::check_launch(where);
}
