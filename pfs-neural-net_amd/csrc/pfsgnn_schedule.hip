// pfsgnn_schedule.hip -- the integer schedule of a trained allocation: hard
// visit counts per edge and what follows from them (train.py:50's commented
// scatter(torch.floor(visited), tgt), the "hard counts & diagnostics" branch of
// train.py:74, the rounding to whole visits of train.py:256-257).
//
//   time_e = softplus(decoder_e(x_e)) * scale      (EdgeTime: EdgeLoss's FMA order)
//   v_e = time_e / T[tgt_e]                        (one IEEE division: a floor sits on it)
//   visits_e = (int) floorf(v_e)  |  (int) rintf(v_e)   (half to even, np.round)
//   n_c = sum visits_e over tgt_e = c              (int32: exact, order-free)
//   fiber_time_f = sum (float)visits_e * T[tgt_e] over src_e = f   (fp32 products,
//                  fixed summation order)
//   completeness_c = n_c / (N_c / nfields); utility_g = min_c; over_g = #{f:
//   fiber_time_f > total_time}; worst_g = max_f fiber_time_f
//
// No noise, no sharpness, no seed.  The dense kernel has k_loss_fwd's grid and
// ownership (lane = fiber, 4 waves over the classes of a split, the prefetch
// ring), the sliced one ksl_loss_fwd's (a lane owns an edge, four steps per
// iteration); one finish launch per graph reduces the int32 class partials and
// the fiber partials.  Nothing allocates, synchronises or uses float atomics
// (the sliced class counts are LDS integer adds: order-free, so reproducible).
#include "pfsgnn_common.h"
#include "pfsgnn_loss_core.h"
#include "pfsgnn_mfma.h"
#include "../../include/pfsgnn.h"

#include <cmath>

namespace {

using pfm::SlGeo;
constexpr int MAXC = pfm::SL_MAX_NC;

// wave_sum (pfsgnn_common.h) on int32: every lane gets the total
__device__ __forceinline__ int wave_isum(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);
  return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) +
         (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}
// sum over the lane's row of 16 lanes, in every lane of the row
__device__ __forceinline__ int row_isum16(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);
  return v;
}

// the visit count of an edge and its time; the product is rounded to fp32 on
// its own (no contraction into the fiber sum: fiber_time sums fp32 terms)
struct Visit {
  int n;
  float tt;
};
__device__ __forceinline__ Visit hard_visit(float time, float Ti, int rounding) {
  const float v = time / Ti;
  const float r = rounding ? rintf(v) : floorf(v);
  Visit o;
  o.n = (int)r;
  o.tt = __fmul_rn((float)o.n, Ti);
  return o;
}

template <int F>
__global__ __launch_bounds__(256) void k_schedule(EdgeGeo geo, const float* __restrict__ y,
                                                  const float* __restrict__ sc,
                                                  const float* __restrict__ sh,
                                                  const float* __restrict__ Wd1,
                                                  const float* __restrict__ bd1,
                                                  const float* __restrict__ Wd2,
                                                  const float* __restrict__ bd2,
                                                  const float* __restrict__ ci, float scale,
                                                  int rounding, int mode,
                                                  const int32_t* __restrict__ perm,
                                                  int* __restrict__ visits,
                                                  float* __restrict__ fiber_time,
                                                  int* __restrict__ part) {
  EDGE_PROLOGUE
  __shared__ float scratch[4 * 64];
  __shared__ __attribute__((aligned(16))) DecW<F> dw;
  dw.load(Wd1, bd1, Wd2, bd2);
  __syncthreads();
  float ft = 0.f;
  Y_PREFETCH_DECL(F)
  CLASS_LOOP_BEGIN
    float x[F];
    Y_TAKE(F, x)
    EdgeTime<F> L;
    const float* dwp = dec_base(dw);
    L.run(x, dwp, dwp + F * F, dwp + F * F + F, dwp + F * F + 2 * F, scale);
    const Visit h = hard_visit(L.time, ci[cn], rounding);
    const int vn = fvalid ? h.n : 0;
    ft += fvalid ? h.tt : 0.f;
    if (fvalid) {
      // the caller's edge: canonical, train.py's fiber-major, or a permutation
      const long long u = mode == 2 ? e : (mode == 1 ? eu : (long long)perm[e]);
      visits[u] = vn;
    }
    const int ns = wave_isum(vn);
    if (lane == 0) part[((size_t)gg * geo.NFG + fg) * geo.NC + c] = ns;
  CLASS_LOOP_END
  // fiber time: merge the 4 waves, KS-partial per fiber (k_loss_fwd's order)
  __syncthreads();
  scratch[wave * 64 + lane] = ft;
  __syncthreads();
  if (t < 64 && t < nvalid)
    fiber_time[(size_t)ks * NS + nbase + t] =
        ((scratch[t] + scratch[64 + t]) + scratch[128 + t]) + scratch[192 + t];
}

template <int F>
__global__ __launch_bounds__(256) void ksl_schedule(
    EdgeGeo geo, SlGeo sl, const int* __restrict__ pos_user, const float* __restrict__ y,
    const float* __restrict__ sc, const float* __restrict__ sh, const float* __restrict__ Wd1,
    const float* __restrict__ bd1, const float* __restrict__ Wd2, const float* __restrict__ bd2,
    const float* __restrict__ ci, float scale, int rounding, int* __restrict__ visits,
    float* __restrict__ fiber_time, int* __restrict__ part) {
  SLL_PROLOGUE
  __shared__ int cnt[MAXC];
  __shared__ __attribute__((aligned(16))) DecW<F> dw;
  dw.load(Wd1, bd1, Wd2, bd2);
  for (int i = t; i < MAXC; i += PF_BLOCK) cnt[i] = 0;
  __syncthreads();
  float ft = 0.f;
  // SLL_LOAD_DECL with the position opaque per iteration: the compiler would
  // otherwise keep one 64-bit row address per channel across the loop (2 F VGPRs)
  auto load = [&](int i) {
    SlEdge<F> r;
    r.in = k0 + 4 * i + q4 < k1;
    long long p = p0 + 64ll * i;
    asm volatile("" : "+v"(p));
    r.cls = r.in ? (int)sl.cls[p] : 0xFF;
    r.pos = r.in ? pos_user[p] : -1;
    const float* yp = y + p;
#pragma unroll
    for (int k = 0; k < F; ++k) r.y[k] = r.in ? yp[(long long)k * EP] : 0.f;
    return r;
  };
  SlEdge<F> cur = load(0);
  for (int i = 0; i < nit; ++i) {
    const SlEdge<F> nxt = load(i + 1);
    SLL_STEP(cur)
    float x[F];
#pragma unroll
    for (int k = 0; k < F; ++k) x[k] = sc ? fmaf(cur.y[k], sc[k], sh[k]) : cur.y[k];
    EdgeTime<F> L;
    const float* dwp = dec_base(dw);
    L.run(x, dwp, dwp + F * F, dwp + F * F + F, dwp + F * F + 2 * F, scale);
    const Visit h = hard_visit(L.time, ci[cn], rounding);
    const int vn = ev ? h.n : 0;
    ft += ev ? h.tt : 0.f;
    if (ev) visits[cur.pos] = vn;
    // class counts: LDS integer adds (order-free).  A row of 16 lanes whose
    // edges share one class (complete-like slices) adds its sum once.
    const uint64_t vm = __ballot(ev);
    if (vm != 0) {
      const uint32_t rowm = (uint32_t)(vm >> (lane & 48)) & 0xFFFFu;
      const int first = (lane & 48) + (rowm ? __builtin_ctz(rowm) : 0);
      const int cfirst = __shfl(cl, first);
      if (__ballot(ev && cl != cfirst) == 0) {
        const int s = row_isum16(vn);
        if (j16 == 0 && rowm) atomicAdd(&cnt[cfirst], s);
      } else if (ev) {
        atomicAdd(&cnt[cl], vn);
      }
    }
    cur = nxt;
  }
  // fiber time: the four step groups of a fiber in fixed order, KS-partial per
  // global fiber (ksl_loss_fwd's order; 0 for a fiber without edges)
  {
    const float f0 = __shfl(ft, j16), f1 = __shfl(ft, j16 + 16);
    const float f2 = __shfl(ft, j16 + 32), f3 = __shfl(ft, j16 + 48);
    if (q4 == 0 && fib >= 0) fiber_time[(size_t)ks * NS + fib] = ((f0 + f1) + f2) + f3;
  }
  __syncthreads();
  for (int c = t; c < NC; c += PF_BLOCK) part[(size_t)bx * NC + c] = cnt[c];
}

__device__ __forceinline__ float nan_max(float a, float b) {
  return (a != a) ? a : ((b != b) ? b : (b > a ? b : a));
}

// one block per graph: the integer class reduce over the graph's bpg partial
// rows (dense: one per 64-fiber group; sliced: one per block), completeness
// and its minimum; the KS fiber partials in fixed order, the fibers over
// total_time and the largest fiber time
__global__ __launch_bounds__(256) void k_schedule_finish(
    int NF, int NC, int NT, int bpg, int KS, long long NS, const int* __restrict__ part,
    const float* __restrict__ ftp, const float* __restrict__ ci, float total_time, float nfields,
    int* __restrict__ n_hard, float* __restrict__ fiber_time, float* __restrict__ completeness,
    float* __restrict__ utility, int* __restrict__ over, float* __restrict__ worst) {
  const int g = blockIdx.x, t = threadIdx.x;
  __shared__ float smin[256], smax[256];
  __shared__ int sover[256];
  __shared__ int cnt[256];
  float mn = INFINITY;
  // classes in chunks of 256; within a chunk of ncc classes the 256 threads form
  // 256 / ncc row groups, each summing every (256 / ncc)-th partial row (the
  // loads of a thread are independent: unrolled, they overlap), merged by LDS
  // integer adds
  for (int cb = 0; cb < NC; cb += 256) {
    const int ncc = min(256, NC - cb), nrg = 256 / ncc;
    const int c = t % ncc, rg = t / ncc;
    cnt[t] = 0;
    __syncthreads();
    if (rg < nrg) {
      const int* q = part + (size_t)g * bpg * NC + cb + c;
      int n = 0;
#pragma unroll 8
      for (int b = rg; b < bpg; b += nrg) n += q[(size_t)b * NC];
      atomicAdd(&cnt[c], n);
    }
    __syncthreads();
    if (t < ncc) {
      const long long cn = (long long)g * NC + cb + t;
      const int n = cnt[t];
      const float Ni = ci[NT + cn] / nfields;
      const float comp = (float)n / Ni;
      n_hard[cn] = n;
      completeness[cn] = comp;
      mn = nan_min(mn, comp);
    }
    __syncthreads();
  }
  // (KS == 1: the edge kernel wrote fiber_time itself, ftp is that buffer and
  // nothing is stored here)
  float mx = 0.f;
  int ov = 0;
#pragma unroll 4
  for (int f = t; f < NF; f += 256) {
    const long long n = (long long)g * NF + f;
    float s = ftp[n];
#pragma unroll 4
    for (int k = 1; k < KS; ++k) s += ftp[(size_t)k * NS + n];
    if (KS > 1) fiber_time[n] = s;
    ov += s > total_time ? 1 : 0;
    mx = nan_max(mx, s);
  }
  smin[t] = mn;
  smax[t] = mx;
  sover[t] = ov;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      smin[t] = nan_min(smin[t], smin[t + s]);
      smax[t] = nan_max(smax[t], smax[t + s]);
      sover[t] += sover[t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    utility[g] = smin[0];
    over[g] = sover[0];
    worst[g] = smax[0];
  }
}

struct Ws {
  char* p;
  size_t left;
  void* take(size_t bytes) {
    const size_t b = align256(bytes);
    if (!p || b > left) return nullptr;
    void* r = p;
    p += b;
    left -= b;
    return r;
  }
};

}  // namespace

extern "C" size_t pfsgnn_schedule_args_bytes(void) { return sizeof(pfsgnn_schedule_args); }

extern "C" int pfsgnn_schedule(const pfsgnn_schedule_args* a, void* ws, size_t ws_bytes,
                               void* stream) {
  const char* where = "pfsgnn_schedule";
  PF_REQUIRE(a, where, "null argument struct");
  PF_REQUIRE(!a->sl == !a->pos_user, where,
             "sl and pos_user go together (both set: a sliced general batch; both NULL: complete)");
  PF_REQUIRE(!(a->sl && a->perm), where,
             "sl with perm: a sliced batch maps its edges by pos_user, mode and perm are the "
             "complete batch's");
  PF_REQUIRE(a->sl || (a->mode >= 0 && a->mode <= 2), where, "mode must be 0 (perm), 1 or 2");
  PF_REQUIRE(a->sl || a->mode != 0 || a->perm, where, "mode 0 needs perm");
  PF_REQUIRE(a->rounding == 0 || a->rounding == 1, where, "rounding must be 0 (floor) or 1 (round)");
  const int G = a->G, NF = a->NF, NC = a->NC, F = a->F;
  PF_REQUIRE(F == 8 || F == 10 || F == 16, where, "unsupported Fdim (8, 10, 16)");
  PF_REQUIRE(G > 0 && NF > 0 && NC > 0, where, "need G > 0, NF > 0, NC > 0");
  if (a->sl) {
    const pfsgnn_sliced_t* s = a->sl;
    PF_REQUIRE(s->fib && s->base && s->len && s->cls && s->EP > 0 && s->E > 0 && s->EP >= s->E,
               where, "bad sliced layout");
    int m = 0;
    if (pfsgnn_sliced_max_nc(F, &m) != 0 || m <= 0)
      return pf::fail(where, "sliced layout: the current edge path has no sliced kernels");
    PF_REQUIRE(NC <= m && NC <= MAXC, where,
               "sliced layout: too many classes per graph (pfsgnn_sliced_max_nc)");
  } else {
    PF_REQUIRE((long long)G * NF * NC < (1ll << 31), where, "E too large for int32 edge ids");
  }
  PF_REQUIRE(a->visits && a->n_hard && a->fiber_time && a->completeness && a->utility && a->over &&
                 a->worst,
             where, "null output");
  PF_REQUIRE(a->y && a->Wd1 && a->bd1 && a->Wd2 && a->bd2 && a->ci && (!a->sc == !a->sh), where,
             "null input (sc and sh go together)");
  hipStream_t st = as_stream(stream);
  Ws w{reinterpret_cast<char*>(ws), ws_bytes};
  EdgeGeo geo;
  int bpg;
  if (a->sl) {
    const pfsgnn_sliced_t& s = *a->sl;
    const SlGeo sg{s.fib, s.base, s.len, s.cls, s.pco, s.EP, s.E, s.maxdeg};
    geo = pfm::sl_geo(G, NF, NC, sg);
    bpg = geo.NFG * geo.KS;   // every block holds every class
    int* part = static_cast<int*>(w.take((size_t)G * bpg * NC * sizeof(int)));
    float* ftp = geo.KS == 1 ? a->fiber_time
                             : static_cast<float*>(w.take((size_t)geo.KS * geo.NS * sizeof(float)));
    PF_REQUIRE(part && ftp, where, "workspace too small");
    { pf::Timer tm_("schedule", st);
    LOSS_DISPATCH_F(F, hipLaunchKernelGGL(ksl_schedule<FF>, dim3(geo.nblocks), dim3(256), 0, st, geo,
                                          sg, a->pos_user, a->y, a->sc, a->sh, a->Wd1, a->bd1,
                                          a->Wd2, a->bd2, a->ci, a->scale, a->rounding, a->visits,
                                          ftp, part));
    tm_.end(); }
    hipLaunchKernelGGL(k_schedule_finish, dim3(G), dim3(256), 0, st, NF, NC, G * NC, bpg, geo.KS,
                       geo.NS, part, ftp, a->ci, a->total_time, a->nfields, a->n_hard,
                       a->fiber_time, a->completeness, a->utility, a->over, a->worst);
  } else {
    geo = loss_geo(G, NF, NC);
    bpg = geo.NFG;            // the class splits own disjoint classes
    int* part = static_cast<int*>(w.take((size_t)G * bpg * NC * sizeof(int)));
    float* ftp = geo.KS == 1 ? a->fiber_time
                             : static_cast<float*>(w.take((size_t)geo.KS * geo.NS * sizeof(float)));
    PF_REQUIRE(part && ftp, where, "workspace too small");
    { pf::Timer tm_("schedule", st);
    LOSS_DISPATCH_F(F, hipLaunchKernelGGL(k_schedule<FF>, dim3(edge_grid(geo)), dim3(256), 0, st, geo,
                                          a->y, a->sc, a->sh, a->Wd1, a->bd1, a->Wd2, a->bd2, a->ci,
                                          a->scale, a->rounding, a->mode, a->perm, a->visits, ftp,
                                          part));
    tm_.end(); }
    hipLaunchKernelGGL(k_schedule_finish, dim3(G), dim3(256), 0, st, NF, NC, G * NC, bpg, geo.KS,
                       geo.NS, part, ftp, a->ci, a->total_time, a->nfields, a->n_hard,
                       a->fiber_time, a->completeness, a->utility, a->over, a->worst);
  }
  return pf::check_launch(where);
}
