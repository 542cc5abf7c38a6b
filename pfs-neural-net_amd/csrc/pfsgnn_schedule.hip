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
// No noise, no sharpness, no seed.  Launches: the per-edge time pass of the
// batch's layout (dense_time_pass / sliced_time_pass below, which the budget's
// quotient pass shares) with the visit count as its sink -- k_schedule /
// ksl_schedule; then one finish launch per graph, which reduces the int32
// class partials and the fiber partials and ends in graph_summary (which the
// plan's finish shares).  Nothing allocates, synchronises or uses float atomics
// (the sliced class counts are LDS integer adds: order-free, so reproducible).
#include "pfsgnn_common.h"
#include "pfsgnn_loss_core.h"
#include "pfsgnn_mfma.h"
#include "../../include/pfsgnn.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>

namespace {

using pfm::SlGeo;
constexpr int MAXC = pfm::SL_MAX_NC;

// sum over the lane's row of 16 lanes, in every lane of the row
__device__ __forceinline__ int row_isum16(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);
  return v;
}
// wave_sum (pfsgnn_common.h) on int32: every lane gets the total
__device__ __forceinline__ int wave_isum(int v) {
  v = row_isum16(v);
  return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) +
         (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}

// a class time that gives its edges no visits: zero, negative, infinite or NaN
__device__ __forceinline__ bool inert_T(float T) { return !(T > 0.f) || !(T < INFINITY); }

// ---- the per-edge time pass, once per layout.  A kernel opens with its
// layout's prologue and passes on the block's place; the pass stages
// decoder_e's weights in LDS, walks the block's edges one load ahead, applies
// the input affine and EdgeTime, and hands every edge's time to the kernel's
// sink, in uniform control flow (a sink may use wave-wide operations).  What a
// kernel does with the time -- and its epilogue -- is its own; the passes know
// no kernel.
//
// Dense: k_loss_fwd's grid and ownership (lane = fiber, 4 waves over the
// classes of a split, the prefetch ring); gg .. wave are EDGE_PROLOGUE's.
// sink(time, fvalid, cn, e, eu): the lane's fiber exists, the class's index
// into ci, the edge's canonical index and its fiber-major one.
template <int F, class Sink>
__device__ __forceinline__ void dense_time_pass(
    const EdgeGeo& geo, int gg, int f, bool fvalid, int c0, int c1, int wave,
    const float* __restrict__ y, const float* __restrict__ sc, const float* __restrict__ sh,
    const float* __restrict__ Wd1, const float* __restrict__ bd1, const float* __restrict__ Wd2,
    const float* __restrict__ bd2, float scale, Sink sink) {
  const long long E = geo.E, n = (long long)gg * geo.NF + (fvalid ? f : 0);
  __shared__ __attribute__((aligned(16))) DecW<F> dw;
  dw.load(Wd1, bd1, Wd2, bd2);
  __syncthreads();
  Y_PREFETCH_DECL(F)
  CLASS_LOOP_BEGIN
    float x[F];
    Y_TAKE(F, x)
    sink(edge_time<F>(x, dw, scale), fvalid, cn, e, eu);
  CLASS_LOOP_END
}

// Sliced: ksl_loss_fwd's grid and ownership (a lane owns an edge, four steps
// per iteration), with the loader whose position is opaque; gg .. p0 are
// SLL_PROLOGUE's.  sink(time, ev, cl, cn, edge, slot): SLL_STEP's validity,
// clamped class and index into ci, the SlEdge and its slot in the sliced
// layout.  The barrier after the staging also covers what the kernel put in
// LDS before the call.
template <int F, class Sink>
__device__ __forceinline__ void sliced_time_pass(
    const EdgeGeo& geo, const SlGeo& sl, int gg, int fib, int q4, int k0, int k1, long long p0,
    const int* __restrict__ pos_user, const float* __restrict__ y, const float* __restrict__ sc,
    const float* __restrict__ sh, const float* __restrict__ Wd1, const float* __restrict__ bd1,
    const float* __restrict__ Wd2, const float* __restrict__ bd2, float scale, Sink sink) {
  const int NC = geo.NC, nit = (k1 - k0 + 3) >> 2;
  const long long EP = geo.E, cn0 = (long long)gg * NC;
  __shared__ __attribute__((aligned(16))) DecW<F> dw;
  dw.load(Wd1, bd1, Wd2, bd2);
  __syncthreads();
  SLL_LOAD_OPAQUE_DECL(F)
  SlEdge<F> cur = load(0);
  for (int i = 0; i < nit; ++i) {
    const SlEdge<F> nxt = load(i + 1);
    SLL_STEP(cur)
    float x[F];
#pragma unroll
    for (int k = 0; k < F; ++k) x[k] = sc ? fmaf(cur.y[k], sc[k], sh[k]) : cur.y[k];
    sink(edge_time<F>(x, dw, scale), ev, cl, cn, cur, p0 + 64ll * i);
    cur = nxt;
  }
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
  float ft = 0.f;
  dense_time_pass<F>(geo, gg, f, fvalid, c0, c1, wave, y, sc, sh, Wd1, bd1, Wd2, bd2, scale,
                     [&](float time, bool fvalid, long long cn, long long e, long long eu) {
    const Visit h = hard_visit(time, ci[cn], rounding);
    const int vn = fvalid ? h.n : 0;
    ft += fvalid ? h.tt : 0.f;
    if (fvalid) visits[caller_pos(mode, e, eu, perm)] = vn;
    const int ns = wave_isum(vn);
    const int c = (int)(cn - (long long)gg * geo.NC);
    if (lane == 0) part[((size_t)gg * geo.NFG + fg) * geo.NC + c] = ns;
  });
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
  for (int i = t; i < MAXC; i += PF_BLOCK) cnt[i] = 0;
  float ft = 0.f;
  sliced_time_pass<F>(geo, sl, gg, fib, q4, k0, k1, p0, pos_user, y, sc, sh, Wd1, bd1, Wd2, bd2,
                      scale,
                      [&](float time, bool ev, int cl, long long cn, const SlEdge<F>& ed, long long) {
    const Visit h = hard_visit(time, ci[cn], rounding);
    const int vn = ev ? h.n : 0;
    ft += ev ? h.tt : 0.f;
    if (ev) visits[ed.pos] = vn;
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
  });
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

// a graph's summary from its block of 256 threads: utility = the minimum of
// the threads' completeness minima (a NaN propagates, like torch.min), over =
// the sum of their counts of fibers over total_time, worst = the maximum of
// their fiber-time maxima (from 0; a NaN propagates)
__device__ __forceinline__ void graph_summary(float mn, float mx, int ov, float* utility,
                                              int* over, float* worst) {
  const int g = blockIdx.x, t = threadIdx.x;
  __shared__ float smin[256], smax[256];
  __shared__ int sover[256];
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
  graph_summary(mn, mx, ov, utility, over, worst);
}

// a bump allocator over the caller's workspace (256-byte aligned pieces); `used`
// counts what was asked for, fitting or not: a pass with p = NULL sizes a layout
struct Ws {
  char* p;
  size_t left, used = 0;
  template <class T>
  T* take(size_t n) {
    const size_t b = align256(n * sizeof(T));
    used += b;
    if (!p || b > left) return nullptr;
    T* r = reinterpret_cast<T*>(p);
    p += b;
    left -= b;
    return r;
  }
};

SlGeo sl_of(const pfsgnn_sliced_t& s) {
  return SlGeo{s.fib, s.base, s.len, s.cls, s.pco, s.EP, s.E, s.maxdeg};
}

// a complete batch's edge order
int check_mode(const char* where, int mode, const int32_t* perm) {
  PF_REQUIRE(mode >= 0 && mode <= 2, where, "mode must be 0 (perm), 1 or 2");
  PF_REQUIRE(mode != 0 || perm, where, "mode 0 needs perm");
  return 0;
}
// the batch of an op that reads the edge state: its form (sliced by sl and
// pos_user, or complete by mode and perm), the decoder width, the dimensions
// and what the layout's kernels can hold
int check_batch(const char* where, int G, int NF, int NC, int F, const pfsgnn_sliced_t* sl,
                const int* pos_user, int mode, const int32_t* perm) {
  PF_REQUIRE(!sl == !pos_user, where,
             "sl and pos_user go together (both set: a sliced general batch; both NULL: complete)");
  PF_REQUIRE(!(sl && perm), where,
             "sl with perm: a sliced batch maps its edges by pos_user, mode and perm are the "
             "complete batch's");
  if (int rc = sl ? 0 : check_mode(where, mode, perm)) return rc;
  PF_REQUIRE(F == 8 || F == 10 || F == 16, where, "unsupported Fdim (8, 10, 16)");
  PF_REQUIRE(G > 0 && NF > 0 && NC > 0, where, "need G > 0, NF > 0, NC > 0");
  if (sl) {
    PF_REQUIRE(sl->fib && sl->base && sl->len && sl->cls && sl->EP > 0 && sl->E > 0 &&
                   sl->EP >= sl->E,
               where, "bad sliced layout");
    int m = 0;
    if (pfsgnn_sliced_max_nc(F, &m) != 0 || m <= 0)
      return pf::fail(where, "sliced layout: the current edge path has no sliced kernels");
    PF_REQUIRE(NC <= m && NC <= MAXC, where,
               "sliced layout: too many classes per graph (pfsgnn_sliced_max_nc)");
  } else {
    PF_REQUIRE((long long)G * NF * NC < (1ll << 31), where, "E too large for int32 edge ids");
  }
  return 0;
}

}  // namespace

extern "C" size_t pfsgnn_schedule_args_bytes(void) { return sizeof(pfsgnn_schedule_args); }

extern "C" int pfsgnn_schedule(const pfsgnn_schedule_args* a, void* ws, size_t ws_bytes,
                               void* stream) {
  const char* where = "pfsgnn_schedule";
  PF_REQUIRE(a, where, "null argument struct");
  const int G = a->G, NF = a->NF, NC = a->NC, F = a->F;
  if (int rc = check_batch(where, G, NF, NC, F, a->sl, a->pos_user, a->mode, a->perm)) return rc;
  PF_REQUIRE(a->rounding == 0 || a->rounding == 1, where, "rounding must be 0 (floor) or 1 (round)");
  PF_REQUIRE(a->visits && a->n_hard && a->fiber_time && a->completeness && a->utility && a->over &&
                 a->worst,
             where, "null output");
  PF_REQUIRE(a->y && a->Wd1 && a->bd1 && a->Wd2 && a->bd2 && a->ci && (!a->sc == !a->sh), where,
             "null input (sc and sh go together)");
  hipStream_t st = as_stream(stream);
  // class-partial rows per graph: a sliced block holds every class, the dense
  // class splits own disjoint classes
  const SlGeo sg = a->sl ? sl_of(*a->sl) : SlGeo{};
  const EdgeGeo geo = a->sl ? pfm::sl_geo(G, NF, NC, sg) : loss_geo(G, NF, NC);
  const int bpg = a->sl ? geo.NFG * geo.KS : geo.NFG;
  Ws w{reinterpret_cast<char*>(ws), ws_bytes};
  int* part = w.take<int>((size_t)G * bpg * NC);
  float* ftp = geo.KS == 1 ? a->fiber_time : w.take<float>((size_t)geo.KS * geo.NS);
  PF_REQUIRE(part && ftp, where, "workspace too small");
  { pf::Timer tm_("schedule", st);
  if (a->sl) {
    LOSS_DISPATCH_F(F, hipLaunchKernelGGL(ksl_schedule<FF>, dim3(geo.nblocks), dim3(256), 0, st, geo,
                                          sg, a->pos_user, a->y, a->sc, a->sh, a->Wd1, a->bd1,
                                          a->Wd2, a->bd2, a->ci, a->scale, a->rounding, a->visits,
                                          ftp, part));
  } else {
    LOSS_DISPATCH_F(F, hipLaunchKernelGGL(k_schedule<FF>, dim3(edge_grid(geo)), dim3(256), 0, st, geo,
                                          a->y, a->sc, a->sh, a->Wd1, a->bd1, a->Wd2, a->bd2, a->ci,
                                          a->scale, a->rounding, a->mode, a->perm, a->visits, ftp,
                                          part));
  }
  tm_.end(); }
  hipLaunchKernelGGL(k_schedule_finish, dim3(G), dim3(256), 0, st, NF, NC, G * NC, bpg, geo.KS,
                     geo.NS, part, ftp, a->ci, a->total_time, a->nfields, a->n_hard, a->fiber_time,
                     a->completeness, a->utility, a->over, a->worst);
  return pf::check_launch(where);
}

// ================================================================ budgeted rounding
namespace {
// pfsgnn_schedule_budget (include/pfsgnn.h): largest-remainder apportionment per
// fiber.  Two launches and the finish above:
//   1. the quotient pass (k_budget_quot / ksl_budget_quot: the dense and the
//      sliced time pass above) writes one 32-bit word per edge in
//      canonical or slot order -- the fp32 quotient q_e >= 0 (sign bit clear),
//      or BQ_DONE | 0 for an inert edge or a padding slot -- and quot in the
//      caller's order; with time_in there is no such launch, the selection
//      pass gathers the times itself;
//   2. the selection pass (k_budget_select / ksl_budget_select): a lane owns a
//      fiber.  Dense: the 64 fibers' words staged as an LDS tile [NC][64];
//      sliced: in place in the workspace (a fiber's steps are unbounded).  A
//      word with the sign bit set is final (the count in its low 31 bits), any
//      other is pending; each pick scans the fiber's words for the extreme
//      pending key, decides, and writes the final word back, so no second
//      per-edge state is needed.  The up phase scans only for candidates that
//      still fit: ft only grows, so one that does not fit now never will -- one
//      scan per bump, not one per candidate.
// Budget arithmetic is double through __dadd_rn / __dmul_rn / __dsub_rn: no FMA
// contraction.  (It would not matter for the products, which are exact in
// double -- 24-bit count x 24-bit T -- but a contracted ft + k * T would round
// once where the definition rounds twice when T is not on the 2^-20 grid.)
constexpr int BUDGET_MAX_NC = 192;          // dense: (NC x 64 + NC) LDS words, 48.75 KB
constexpr uint32_t BQ_DONE = 0x80000000u;

__device__ __forceinline__ uint32_t budget_word(float time, float Ti, float* q_out) {
  const float v = time / Ti;                 // one IEEE division
  const bool inert = !(v == v) || inert_T(Ti);
  const float q = inert ? 0.f : (v > 0.f ? fminf(v, 16777216.f) : 0.f);
  *q_out = q;
  return inert ? BQ_DONE : __float_as_uint(q);
}
__device__ __forceinline__ int budget_final(uint32_t w) {
  return (w & BQ_DONE) ? (int)(w & ~BQ_DONE) : (int)floorf(__uint_as_float(w));
}

template <int F>
__global__ __launch_bounds__(256) void k_budget_quot(
    EdgeGeo geo, const float* __restrict__ y, const float* __restrict__ sc,
    const float* __restrict__ sh, const float* __restrict__ Wd1, const float* __restrict__ bd1,
    const float* __restrict__ Wd2, const float* __restrict__ bd2, const float* __restrict__ ci,
    float scale, int mode, const int32_t* __restrict__ perm, uint32_t* __restrict__ qws,
    float* __restrict__ quot) {
  EDGE_PROLOGUE
  dense_time_pass<F>(geo, gg, f, fvalid, c0, c1, wave, y, sc, sh, Wd1, bd1, Wd2, bd2, scale,
                     [&](float time, bool fvalid, long long cn, long long e, long long eu) {
    float q;
    const uint32_t w = budget_word(time, ci[cn], &q);
    if (fvalid) {
      qws[e] = w;                            // canonical: consecutive fibers, coalesced
      if (quot) quot[caller_pos(mode, e, eu, perm)] = q;
    }
  });
}

template <int F>
__global__ __launch_bounds__(256) void ksl_budget_quot(
    EdgeGeo geo, SlGeo sl, const int* __restrict__ pos_user, const float* __restrict__ y,
    const float* __restrict__ sc, const float* __restrict__ sh, const float* __restrict__ Wd1,
    const float* __restrict__ bd1, const float* __restrict__ Wd2, const float* __restrict__ bd2,
    const float* __restrict__ ci, float scale, uint32_t* __restrict__ qws,
    float* __restrict__ quot) {
  SLL_PROLOGUE
  sliced_time_pass<F>(geo, sl, gg, fib, q4, k0, k1, p0, pos_user, y, sc, sh, Wd1, bd1, Wd2, bd2,
                      scale,
                      [&](float time, bool ev, int, long long cn, const SlEdge<F>& ed, long long slot) {
    float q;
    const uint32_t w = budget_word(time, ci[cn], &q);
    // every slot of the split is written: padding and fiber-less lanes as final 0
    if (ed.in) qws[slot] = ev ? w : BQ_DONE;
    if (ev && quot) quot[ed.pos] = q;
  });
}

// the words of the lane's fiber: dense, column `lane` of the LDS tile (step k =
// class k); sliced, the slots base + 16 k + j of the workspace, their class
// bytes and caller positions
struct DenseTile {
  uint32_t* w;
  int n;
  __device__ __forceinline__ uint32_t get(int k) const { return w[k * 64]; }
  __device__ __forceinline__ void put(int k, uint32_t v) const { w[k * 64] = v; }
  __device__ __forceinline__ int cls(int k) const { return k; }
  __device__ __forceinline__ int pos(int k) const { return k; }
};
struct SlicedTile {
  uint32_t* w;
  const uint8_t* c;
  const int* p;
  int n;
  __device__ __forceinline__ uint32_t get(int k) const { return w[16 * k]; }
  __device__ __forceinline__ void put(int k, uint32_t v) const { w[16 * k] = v; }
  __device__ __forceinline__ int cls(int k) const { return c[16 * k]; }
  __device__ __forceinline__ int pos(int k) const { return p[16 * k]; }
};

struct Pick {
  int k, c;
  float q;
};
// the pending edge with the extreme key (frac, class, caller position).  DOWN:
// the smallest frac among those with a visit to lose.  Else the largest frac
// among those that still fit, ft + T <= tot: ft only grows, so a candidate that
// does not fit now never will, and the walk in descending key order would have
// refused it -- skipping it here is the same walk with one scan per bump
// instead of one per candidate; *unfit: a pending edge was passed over so.
// Ties to the lower class, then the lower position.  k < 0: none
template <bool DOWN, class Tile>
__device__ __forceinline__ Pick budget_scan(const Tile& tl, int nmax, const float* Ts, double ft,
                                            double tot, bool* unfit) {
  Pick b{-1, 0, 0.f};
  float bf = 0.f;
  bool uf = false;
  // branch-free per word (selects; the loads of an unrolled group issue
  // together): a wave is alone on its SIMD here, nothing else hides a branchy
  // body's LDS latency.  Only a (frac, class) tie -- a repeated pair -- branches
#pragma unroll 4
  for (int k = 0; k < nmax; ++k) {
    const bool in = k < tl.n;
    const uint32_t w = in ? tl.get(k) : BQ_DONE;
    const bool pend = !(w & BQ_DONE);
    const float q = __uint_as_float(w), fl = floorf(q), f = q - fl;   // exact in fp32
    const int c = pend ? tl.cls(k) : 0;      // (a pending word has a class < NC)
    bool cand;
    if (DOWN) {
      cand = pend && fl >= 1.f;
    } else {
      const bool fits = __dadd_rn(ft, (double)Ts[c]) <= tot;
      cand = pend && fits;
      uf |= pend && !fits;
    }
    bool better = b.k < 0 || (DOWN ? f < bf : f > bf) || (f == bf && c < b.c);
    if (cand && !better && f == bf && c == b.c) better = tl.pos(k) < tl.pos(b.k);
    const bool take = cand && better;
    b.k = take ? k : b.k;
    b.c = take ? c : b.c;
    b.q = take ? q : b.q;
    bf = take ? f : bf;
  }
  *unfit = uf;
  return b;
}

// both phases on the lane's fiber; ft the double sum of floor(q) * T over its
// pending edges.  -> the phase bits
template <class Tile>
__device__ __forceinline__ int budget_round_fiber(const Tile& tl, int nmax, const float* Ts,
                                                  double ft, double tot) {
  int ph = 0;
  bool unfit = false;
  if (ft > tot) {
    ph |= 1;
    while (ft > tot) {
      const Pick b = budget_scan<true>(tl, nmax, Ts, ft, tot, &unfit);
      if (b.k < 0) break;
      const double Td = (double)Ts[b.c];
      const int vis = (int)floorf(b.q);
      // the smallest k with ft - k T <= tot: ceil of the quotient, then one
      // exact step either way; beyond any count the edge is stripped
      double kd = ceil(__dsub_rn(ft, tot) / Td);
      if (!(kd < 33554432.0)) kd = 33554432.0;
      if (kd >= 1.0 && __dsub_rn(ft, __dmul_rn(kd - 1.0, Td)) <= tot) kd -= 1.0;
      else if (__dsub_rn(ft, __dmul_rn(kd, Td)) > tot) kd += 1.0;
      const int r = kd < (double)vis ? (int)kd : vis;
      ft = __dsub_rn(ft, __dmul_rn((double)r, Td));
      tl.put(b.k, BQ_DONE | (uint32_t)(vis - r));
    }
  }
  for (;;) {
    unfit = false;
    const Pick b = budget_scan<false>(tl, nmax, Ts, ft, tot, &unfit);
    if (b.k < 0) break;                        // (what is left pending keeps its floor)
    ft = __dadd_rn(ft, (double)Ts[b.c]);       // equality fits
    ph |= 2;
    tl.put(b.k, BQ_DONE | (uint32_t)((int)floorf(b.q) + 1));
  }
  return ph | (unfit ? 4 : 0);
}

// one wave per 64 fibers of a graph; dynamic LDS: Ts [NC rounded up to 64] |
// tile [NC][64]
__global__ __launch_bounds__(64) void k_budget_select(
    int NF, int NC, int NFG, const uint32_t* __restrict__ qws, const float* __restrict__ time_in,
    const float* __restrict__ ci, float total_time, int mode, const int32_t* __restrict__ perm,
    int* __restrict__ visits, float* __restrict__ quot, float* __restrict__ fiber_time,
    int* __restrict__ phase, int* __restrict__ part) {
  extern __shared__ uint32_t budget_lds[];
  const int lane = threadIdx.x, gg = blockIdx.x / NFG, fg = blockIdx.x % NFG;
  float* Ts = reinterpret_cast<float*>(budget_lds);
  for (int c = lane; c < NC; c += 64) Ts[c] = ci[(long long)gg * NC + c];
  __syncthreads();
  const int f = fg * 64 + lane;
  const bool fvalid = f < NF;
  const long long n = (long long)gg * NF + (fvalid ? f : 0);
  // (a lane beyond NF holds final zeros: its column takes part in every walk)
  const DenseTile tl{budget_lds + ((NC + 63) & ~63) + lane, NC};
  const long long e0 = (long long)gg * NC * NF + (fvalid ? f : 0);
  auto user = [&](int k) {
    const long long e = e0 + (long long)k * NF;
    return caller_pos(mode, e, n * NC + k, perm);
  };
  double ft = 0.0;
  if (time_in) {
    for (int k = 0; k < NC; ++k) {
      const long long u = user(k);
      float q;
      const uint32_t w = budget_word(time_in[u], Ts[k], &q);
      if (fvalid && quot) quot[u] = q;
      tl.put(k, fvalid ? w : BQ_DONE);
    }
  } else {
    // canonical words: consecutive fibers; unconditional loads (a lane beyond NF
    // re-reads fiber 0's), so that an unrolled group's loads are in flight together
#pragma unroll 8
    for (int k = 0; k < NC; ++k) tl.put(k, fvalid ? qws[e0 + (long long)k * NF] : BQ_DONE);
  }
#pragma unroll 4
  for (int k = 0; k < NC; ++k) {
    const uint32_t w = tl.get(k);
    const double t = __dmul_rn((double)floorf(__uint_as_float(w)), (double)Ts[k]);
    ft = (w & BQ_DONE) ? ft : __dadd_rn(ft, t);
  }
  const int ph = budget_round_fiber(tl, NC, Ts, ft, (double)total_time);
  // counts out in class order: the class partial of the 64 fibers, the fp32
  // fiber time (fp32 products, ascending class)
  float ft32 = 0.f;
  for (int k = 0; k < NC; ++k) {
    const int v = fvalid ? budget_final(tl.get(k)) : 0;
    if (fvalid) {
      visits[user(k)] = v;
      if (v) ft32 = __fadd_rn(ft32, __fmul_rn((float)v, Ts[k]));
    }
    const int ns = wave_isum(v);
    if (lane == 0) part[((size_t)gg * NFG + fg) * NC + k] = ns;
  }
  if (fvalid) {
    fiber_time[n] = ft32;
    phase[n] = ph;
  }
}

// one wave per group of 4 slices (64 fiber lanes of a graph)
__global__ __launch_bounds__(64) void ksl_budget_select(
    SlGeo sl, int NC, int NFG, const int* __restrict__ pos_user, uint32_t* qws,
    const float* __restrict__ time_in, const float* __restrict__ ci, float total_time,
    int* __restrict__ visits, float* __restrict__ quot, float* __restrict__ fiber_time,
    int* __restrict__ phase, int* __restrict__ part) {
  __shared__ float Ts[MAXC];
  __shared__ int cnt[MAXC];
  const int lane = threadIdx.x, grp = blockIdx.x, gg = grp / NFG;
  for (int c = lane; c < MAXC; c += 64) {
    Ts[c] = c < NC ? ci[(long long)gg * NC + c] : 0.f;
    cnt[c] = 0;
  }
  __syncthreads();
  const int slc = 4 * grp + (lane >> 4), j = lane & 15;
  const int fib = sl.fib[slc * 16 + j];
  const long long pb = (long long)sl.base[slc] + j;
  const int n = fib >= 0 ? sl.len[slc] : 0;
  int nmax = n;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nmax = max(nmax, __shfl_xor(nmax, o));
  const SlicedTile tl{qws + pb, sl.cls + pb, pos_user + pb, n};
  double ft = 0.0;
  for (int k = 0; k < nmax; ++k) {
    if (k >= n) continue;
    uint32_t w;
    if (time_in) {
      const int c = tl.cls(k), p = tl.pos(k);
      w = BQ_DONE;
      if (c < NC && p >= 0) {
        float q;
        w = budget_word(time_in[p], Ts[c], &q);
        if (quot) quot[p] = q;
      }
      tl.put(k, w);
    } else {
      w = tl.get(k);
    }
    if (!(w & BQ_DONE))
      ft = __dadd_rn(ft, __dmul_rn((double)floorf(__uint_as_float(w)), (double)Ts[tl.cls(k)]));
  }
  const int ph = budget_round_fiber(tl, nmax, Ts, ft, (double)total_time);
  float ft32 = 0.f;
  for (int k = 0; k < nmax; ++k) {
    if (k >= n) continue;
    const int c = tl.cls(k), p = tl.pos(k);
    if (c >= NC || p < 0) continue;
    const int v = budget_final(tl.get(k));
    visits[p] = v;
    if (v) {
      ft32 = __fadd_rn(ft32, __fmul_rn((float)v, Ts[c]));
      atomicAdd(&cnt[c], v);                 // LDS integer add: order-free
    }
  }
  if (fib >= 0) {
    fiber_time[fib] = ft32;
    phase[fib] = ph;
  }
  __syncthreads();
  for (int c = lane; c < NC; c += 64) part[(size_t)grp * NC + c] = cnt[c];
}

size_t budget_ws_bytes(long long slots, int G, int NF, int NC) {
  const size_t NFG = (NF + 63) / 64;
  return align256((size_t)slots * sizeof(uint32_t)) + align256((size_t)G * NFG * NC * sizeof(int));
}

}  // namespace

extern "C" size_t pfsgnn_schedule_budget_args_bytes(void) {
  return sizeof(pfsgnn_schedule_budget_args);
}
extern "C" int pfsgnn_schedule_budget_max_nc(void) { return BUDGET_MAX_NC; }
extern "C" size_t pfsgnn_schedule_budget_ws_bytes(int G, int NF, int NC, long long EP) {
  if (G <= 0 || NF <= 0 || NC <= 0) return 0;
  return budget_ws_bytes(EP > 0 ? EP : (long long)G * NF * NC, G, NF, NC);
}

extern "C" int pfsgnn_schedule_budget(const pfsgnn_schedule_budget_args* a, void* ws,
                                      size_t ws_bytes, void* stream) {
  const char* where = "pfsgnn_schedule_budget";
  PF_REQUIRE(a, where, "null argument struct");
  const int G = a->G, NF = a->NF, NC = a->NC, F = a->F;
  if (int rc = check_batch(where, G, NF, NC, F, a->sl, a->pos_user, a->mode, a->perm)) return rc;
  if (a->sl) {
    PF_REQUIRE(a->sl->EP < (1ll << 31), where, "EP too large for int32 slot ids");
  } else {
    PF_REQUIRE(NC <= BUDGET_MAX_NC, where,
               "too many classes per graph for the selection pass's LDS tile "
               "(pfsgnn_schedule_budget_max_nc)");
  }
  PF_REQUIRE(a->visits && a->n_hard && a->fiber_time && a->completeness && a->utility && a->over &&
                 a->worst && a->phase,
             where, "null output");
  PF_REQUIRE(a->ci && (a->time_in || (a->y && a->Wd1 && a->bd1 && a->Wd2 && a->bd2 &&
                                      (!a->sc == !a->sh))),
             where, "null input (without time_in: y and the decoder; sc and sh go together)");
  hipStream_t st = as_stream(stream);
  Ws w{reinterpret_cast<char*>(ws), ws_bytes};
  const int NFG = (NF + 63) / 64;
  const long long slots = a->sl ? a->sl->EP : (long long)G * NF * NC;
  uint32_t* qws = w.take<uint32_t>((size_t)slots);
  int* part = w.take<int>((size_t)G * NFG * NC);
  PF_REQUIRE(qws && part, where, "workspace too small (pfsgnn_schedule_budget_ws_bytes)");
  if (a->sl) {
    const SlGeo sg = sl_of(*a->sl);
    if (!a->time_in) {
      const EdgeGeo geo = pfm::sl_geo(G, NF, NC, sg);
      LOSS_DISPATCH_F(F, hipLaunchKernelGGL(ksl_budget_quot<FF>, dim3(geo.nblocks), dim3(256), 0, st,
                                            geo, sg, a->pos_user, a->y, a->sc, a->sh, a->Wd1, a->bd1,
                                            a->Wd2, a->bd2, a->ci, a->scale, qws, a->quot));
    }
    hipLaunchKernelGGL(ksl_budget_select, dim3(G * NFG), dim3(64), 0, st, sg, NC, NFG, a->pos_user,
                       qws, a->time_in, a->ci, a->total_time, a->visits, a->quot, a->fiber_time,
                       a->phase, part);
  } else {
    if (!a->time_in) {
      const EdgeGeo geo = loss_geo(G, NF, NC);
      LOSS_DISPATCH_F(F, hipLaunchKernelGGL(k_budget_quot<FF>, dim3(edge_grid(geo)), dim3(256), 0, st,
                                            geo, a->y, a->sc, a->sh, a->Wd1, a->bd1, a->Wd2, a->bd2,
                                            a->ci, a->scale, a->mode, a->perm, qws, a->quot));
    }
    const size_t lds = ((size_t)((NC + 63) & ~63) + (size_t)NC * 64) * sizeof(uint32_t);
    hipLaunchKernelGGL(k_budget_select, dim3(G * NFG), dim3(64), lds, st, NF, NC, NFG, qws,
                       a->time_in, a->ci, a->total_time, a->mode, a->perm, a->visits, a->quot,
                       a->fiber_time, a->phase, part);
  }
  // the selection pass owns whole fibers: one fiber-time row, NFG class partial rows
  hipLaunchKernelGGL(k_schedule_finish, dim3(G), dim3(256), 0, st, NF, NC, G * NC, NFG, 1,
                     (long long)G * NF, part, a->fiber_time, a->ci, a->total_time, a->nfields,
                     a->n_hard, a->fiber_time, a->completeness, a->utility, a->over, a->worst);
  return pf::check_launch(where);
}

// ================================================================ observing plan
namespace {
// pfsgnn_schedule_plan (include/pfsgnn.h): class-capped visits, fiber timelines
// and the target list.  The edge state is never read; the op's working set is
// one int32 word per edge (the sanitised, then trimmed, visit count) in
// canonical order (complete: a class's NF words contiguous) or in CSR position
// order (general: a class's words gathered through cls_ord, a fiber's through
// the plan order below).  Launches:
//   general only: k_plan_keys + one stable radix sort of cls_ord -- (tgt, src,
//      position) order -- by src: the plan order (src, tgt, position), whose
//      fiber runs are fib_ptr's;
//   1. k_plan_class, a block per class: gather + sanitise (the one read of
//      visits_in), the int64 class sum, and for a class over its cap the level
//      L by bisection (int64 block sums over the class's words: in LDS up to
//      PLAN_LDS of them, else re-read by the thread that wrote them) and the
//      ranks of the edges above the level by ballot scans in edge order;
//   2. k_plan_fiber<false> (complete: a lane per fiber walking its classes with
//      a double running sum) / k_plan_fiber_csr<false> (general: a wave per
//      fiber, 64 edges of its plan-order run per step, wave scans of the double
//      durations and the int64 counts -- a hub's degree has no bound): visits,
//      start, used, idle, the fiber's count and its over flag;
//   3. k_plan_finish, a block per graph; one device scan of the counts;
//   4. the same fiber kernels with FILL: the walk again, writing the segments.
constexpr int PLAN_LDS = 8192;
constexpr int PLAN_WMAX = 1 << 24;

// sum / max over the block of 256 in every thread (red: 4 words of LDS)
__device__ __forceinline__ long long plan_block_sum(long long v, long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ int plan_block_max(int v, long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (int)max(max(red[0], red[1]), max(red[2], red[3]));
}

__global__ __launch_bounds__(256) void k_plan_keys(long long E, const int* __restrict__ src_p,
                                                   const int* __restrict__ cls_ord,
                                                   int* __restrict__ key) {
  for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < E;
       k += (long long)gridDim.x * 256)
    key[k] = src_p[cls_ord[k]];
}

template <bool CSR>
__global__ __launch_bounds__(256) void k_plan_class(
    int NF, int NC, int NT, int mode, const int32_t* __restrict__ perm,
    const int* __restrict__ cls_ord, const int* __restrict__ cls_ptr,
    const int* __restrict__ user_of, const float* __restrict__ ci, float nfields, int cap,
    const int32_t* __restrict__ visits_in, int* w, int32_t* __restrict__ n_hard,
    float* __restrict__ completeness, long long* __restrict__ cut) {
  __shared__ int lw[PLAN_LDS];
  __shared__ long long red[4];
  __shared__ int wtot[4];
  const int cn = blockIdx.x, t = threadIdx.x;
  const int gg = cn / NC, c = cn - gg * NC;
  const float T = ci[cn];
  const bool inert = inert_T(T);
  long long k0;
  int n;
  if (CSR) {
    k0 = cls_ptr[cn];
    n = cls_ptr[cn + 1] - (int)k0;
  } else {
    k0 = ((long long)gg * NC + c) * NF;
    n = NF;
  }
  // edge k of the class, in ascending (src, caller position) order: its word
  auto slot = [&](int k) -> long long { return CSR ? (long long)cls_ord[k0 + k] : k0 + k; };
  const bool inl = n <= PLAN_LDS;
  auto get = [&](int k) -> int { return inl ? lw[k] : w[slot(k)]; };
  // (a thread only ever re-reads the words it wrote: k = t mod 256 throughout)
  long long S = 0;
  int mx = 0;
  for (int k = t; k < n; k += 256) {
    const long long s = slot(k);
    long long u;
    if (CSR) u = user_of[s];
    else u = caller_pos(mode, s, ((long long)gg * NF + k) * NC + c, perm);
    int v = visits_in[u];
    v = inert ? 0 : min(max(v, 0), PLAN_WMAX);
    w[s] = v;
    if (inl) lw[k] = v;
    S += v;
    mx = max(mx, v);
  }
  S = plan_block_sum(S, red);
  const float Ni = ci[NT + cn] / nfields;      // one IEEE division
  long long capc = 0;
  bool capped = cap != 0;
  if (Ni != Ni || Ni < 0.f) capc = 0;
  else if (Ni >= 2147483648.f) capped = false;
  else capc = (long long)floorf(Ni);
  long long nfin = S, cutc = 0;
  if (capped && S > capc) {                    // (block-uniform)
    mx = plan_block_max(mx, red);
    // f(L) = sum min(w, L): f(0) = 0 <= cap, f(mx) = S > cap
    int lo = 0, hi = mx;
    long long flo = 0;
    while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      long long s = 0;
      for (int k = t; k < n; k += 256) s += min(get(k), mid);
      s = plan_block_sum(s, red);
      if (s <= capc) {
        lo = mid;
        flo = s;
      } else {
        hi = mid;
      }
    }
    const int L = lo;
    const long long rem = capc - flo;
    // the edges above the level, ranked in edge order: the first rem keep L + 1
    const int lane = t & 63, wv = t >> 6;
    long long carry = 0;
    for (int kb = 0; kb < n; kb += 256) {
      const int k = kb + t;
      const bool above = k < n && get(k) > L;
      const unsigned long long b = __ballot(above);
      const int inw = __popcll(b & ((1ull << lane) - 1ull));
      __syncthreads();
      if (lane == 0) wtot[wv] = __popcll(b);
      __syncthreads();
      long long rank = carry + inw;
      for (int j = 0; j < wv; ++j) rank += wtot[j];
      if (above) w[slot(k)] = L + (rank < rem ? 1 : 0);
      carry += (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
    }
    nfin = capc;
    cutc = S - capc;
  }
  if (t == 0) {
    n_hard[cn] = (int32_t)nfin;
    completeness[cn] = (float)(int32_t)nfin / Ni;
    cut[cn] = cutc;
  }
}

struct PlanOut {
  int32_t* visits;
  float *start, *used, *idle;
  long long* cnt;
  int* ovf;
  const long long* seg_ptr;
  long long seg_cap;
  int32_t* seg_edge;
  float* seg_start;
};

// visit m of an edge with v visits: at i0 + m, start + m T in double
__device__ __forceinline__ void plan_fill(const PlanOut& o, long long i0, int v, int u, double st,
                                          double Td) {
  for (int m = 0; m < v; ++m) {
    const long long i = i0 + m;
    if (i >= o.seg_cap) break;
    o.seg_edge[i] = u;
    o.seg_start[i] = (float)(st + (double)m * Td);   // (m T exact: 24 x 24 bits)
  }
}

template <bool FILL>
__global__ __launch_bounds__(256) void k_plan_fiber(int NF, int NC, int NFB, long long NS, int mode,
                                                    const int32_t* __restrict__ perm,
                                                    const int* __restrict__ w,
                                                    const float* __restrict__ ci, float total_time,
                                                    PlanOut o) {
  const int gg = blockIdx.x / NFB, f = (blockIdx.x - gg * NFB) * 256 + threadIdx.x;
  if (f >= NF) return;
  const long long n = (long long)gg * NF + f;
  const long long e0 = (long long)gg * NC * NF + f;
  const float* Tg = ci + (long long)gg * NC;
  double run = 0.0;
  long long c = 0;
  const long long i0 = FILL ? o.seg_ptr[n] : 0;
#pragma unroll 4
  for (int k = 0; k < NC; ++k) {
    const long long e = e0 + (long long)k * NF;   // canonical: consecutive fibers, coalesced
    const int v = w[e];
    const long long u = caller_pos(mode, e, n * NC + k, perm);
    const double Td = (double)Tg[k];
    if (FILL) {
      plan_fill(o, i0 + c, v, (int)u, run, Td);
    } else {
      o.visits[u] = v;
      o.start[u] = (float)run;
    }
    if (v) run += (double)v * Td;                 // (exact product; an inert T never enters)
    c += v;
  }
  if (!FILL) {
    o.used[n] = (float)run;
    o.idle[n] = (float)((double)total_time - run);
    o.cnt[n] = c;
    o.ovf[n] = run > (double)total_time ? 1 : 0;
    if (n == 0) o.cnt[NS] = 0;
  }
}

template <bool FILL>
__global__ __launch_bounds__(256) void k_plan_fiber_csr(
    long long NS, const int* __restrict__ fib_ptr, const int* __restrict__ pord,
    const int* __restrict__ tgt_p, const int* __restrict__ user_of, const int* __restrict__ w,
    const float* __restrict__ ci, float total_time, PlanOut o) {
  const int lane = threadIdx.x & 63;
  const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= NS) return;                            // the whole wave
  const int p0 = fib_ptr[n], p1 = fib_ptr[n + 1];
  double run = 0.0;
  long long c = 0;
  const long long i0 = FILL ? o.seg_ptr[n] : 0;
  for (int kb = p0; kb < p1; kb += 64) {
    const int k = kb + lane;
    const bool in = k < p1;
    const int p = in ? pord[k] : 0;
    const int v = in ? w[p] : 0;
    const int u = in ? user_of[p] : 0;
    const double Td = in ? (double)ci[tgt_p[p]] : 0.0;
    // inclusive wave scans of the duration and the count, in plan order
    double ds = v ? (double)v * Td : 0.0;
    long long cs = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const double d2 = __shfl_up(ds, s);
      const long long c2 = __shfl_up(cs, s);
      if (lane >= s) {
        ds += d2;
        cs += c2;
      }
    }
    double de = __shfl_up(ds, 1);
    long long ce = __shfl_up(cs, 1);
    if (lane == 0) {
      de = 0.0;
      ce = 0;
    }
    const double st = run + de;
    if (in) {
      if (FILL) {
        plan_fill(o, i0 + c + ce, v, u, st, Td);
      } else {
        o.visits[u] = v;
        o.start[u] = (float)st;
      }
    }
    run += __shfl(ds, 63);
    c += __shfl(cs, 63);
  }
  if (!FILL && lane == 0) {
    o.used[n] = (float)run;
    o.idle[n] = (float)((double)total_time - run);
    o.cnt[n] = c;
    o.ovf[n] = run > (double)total_time ? 1 : 0;
    if (n == 0) o.cnt[NS] = 0;
  }
}

// a block per graph: utility = min completeness, the fibers over, the largest used
__global__ __launch_bounds__(256) void k_plan_finish(int NF, int NC,
                                                     const float* __restrict__ completeness,
                                                     const float* __restrict__ used,
                                                     const int* __restrict__ ovf,
                                                     float* __restrict__ utility,
                                                     int* __restrict__ over,
                                                     float* __restrict__ worst) {
  const int g = blockIdx.x, t = threadIdx.x;
  float mn = INFINITY, mx = 0.f;
  int ov = 0;
  for (int c = t; c < NC; c += 256) mn = nan_min(mn, completeness[(long long)g * NC + c]);
  for (int f = t; f < NF; f += 256) {
    const long long n = (long long)g * NF + f;
    mx = nan_max(mx, used[n]);
    ov += ovf[n];
  }
  graph_summary(mn, mx, ov, utility, over, worst);
}

int plan_key_bits(long long n) {  // keys are 0..n-1
  int b = 1;
  while (b < 31 && (1ll << b) < n) ++b;
  return b;
}

// the op's workspace: the words (general: the sort's input keys first, dead
// once it has run), general only the sort's output keys and the plan order,
// the fibers' counts (+ 1: the scan's total), their over flags, hipcub's scratch
struct PlanWs {
  int *w, *keyB, *pord;
  long long* cnt;
  int* ovf;
  char* tmp;
  size_t tmp_bytes;
};
PlanWs plan_ws(Ws& ws, int G, int NF, int NC, long long E) {   // E = 0: a complete batch
  const long long NS = (long long)G * NF;
  const bool csr = E > 0;
  const long long edges = csr ? E : NS * NC;
  size_t tscan = 0, tsort = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tscan, (const long long*)nullptr,
                                         (long long*)nullptr, (int)(NS + 1));
  if (csr)
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tsort, (const int*)nullptr, (int*)nullptr,
                                             (const int*)nullptr, (int*)nullptr, (int)edges);
  PlanWs p;
  p.w = ws.take<int>((size_t)edges);
  p.keyB = csr ? ws.take<int>((size_t)edges) : nullptr;
  p.pord = csr ? ws.take<int>((size_t)edges) : nullptr;
  p.cnt = ws.take<long long>((size_t)(NS + 1));
  p.ovf = ws.take<int>((size_t)NS);
  p.tmp_bytes = align256(std::max(tscan, tsort)) + 256;
  p.tmp = ws.take<char>(p.tmp_bytes);
  return p;
}

}  // namespace

extern "C" size_t pfsgnn_schedule_plan_args_bytes(void) { return sizeof(pfsgnn_schedule_plan_args); }

extern "C" size_t pfsgnn_schedule_plan_ws_bytes(int G, int NF, int NC, long long E) {
  if (G <= 0 || NF <= 0 || NC <= 0 || E < 0 || E >= (1ll << 31) ||
      (long long)G * NF >= (1ll << 31) - 1 || (E == 0 && (long long)G * NF * NC >= (1ll << 31)))
    return 0;
  Ws sizing{nullptr, 0};
  plan_ws(sizing, G, NF, NC, E);
  return sizing.used;
}

extern "C" int pfsgnn_schedule_plan(const pfsgnn_schedule_plan_args* a, void* ws, size_t ws_bytes,
                                    void* stream) {
  const char* where = "pfsgnn_schedule_plan";
  PF_REQUIRE(a, where, "null argument struct");
  const bool any_csr = a->src_p || a->tgt_p || a->user_of || a->fib_ptr || a->cls_ord || a->cls_ptr;
  const bool complete = a->mode != -1 || a->perm;
  PF_REQUIRE(!(complete && any_csr), where,
             "both batch forms: a complete batch (mode 0..2, perm) leaves the CSR arrays NULL, a "
             "general batch sets mode = -1 and no perm");
  PF_REQUIRE(complete || any_csr, where,
             "neither batch form: mode = -1 needs the CSR arrays of pfsgnn_sparse_layout");
  if (complete) {
    if (int rc = check_mode(where, a->mode, a->perm)) return rc;
  } else {
    PF_REQUIRE(a->src_p && a->tgt_p && a->user_of && a->fib_ptr && a->cls_ord && a->cls_ptr, where,
               "the CSR form needs src_p, tgt_p, user_of, fib_ptr, cls_ord and cls_ptr");
  }
  PF_REQUIRE(a->visits && a->start && a->used && a->idle && a->n_hard && a->completeness &&
                 a->utility && a->over && a->worst && a->cut && a->seg_ptr,
             where, "null output (only seg_edge and seg_start may be NULL)");
  PF_REQUIRE(a->ci && a->visits_in, where, "null input (ci, visits_in)");
  PF_REQUIRE(a->seg_cap >= 0, where, "seg_cap must be >= 0");
  PF_REQUIRE(a->seg_cap == 0 || (a->seg_edge && a->seg_start), where,
             "seg_cap > 0 needs seg_edge and seg_start");
  PF_REQUIRE(a->cap == 0 || a->cap == 1, where, "cap must be 0 or 1");
  const int G = a->G, NF = a->NF, NC = a->NC;
  PF_REQUIRE(G > 0 && NF > 0 && NC > 0 && (complete || a->E > 0), where,
             "need G > 0, NF > 0, NC > 0 (and E > 0 in the CSR form)");
  const long long NS = (long long)G * NF, NT = (long long)G * NC;
  const long long E = complete ? NS * NC : a->E;
  PF_REQUIRE(E < (1ll << 31) && NS < (1ll << 31) - 1 && NT < (1ll << 31), where,
             "E too large for int32 edge ids (E, G*NF, G*NC < 2^31)");
  Ws wsp{static_cast<char*>(ws), ws_bytes};
  const PlanWs p = plan_ws(wsp, G, NF, NC, complete ? 0 : E);
  PF_REQUIRE(ws && wsp.used <= ws_bytes, where,
             "workspace too small (pfsgnn_schedule_plan_ws_bytes)");
  hipStream_t st = as_stream(stream);
  const bool fill = a->seg_cap > 0;
  PlanOut o{a->visits, a->start, a->used, a->idle, p.cnt, p.ovf, a->seg_ptr, a->seg_cap,
            a->seg_edge, a->seg_start};
  const unsigned egrid = (unsigned)std::max<long long>(1, std::min<long long>((E + 255) / 256, 8192));
  if (!complete) {
    hipLaunchKernelGGL(k_plan_keys, dim3(egrid), dim3(256), 0, st, E, a->src_p, a->cls_ord, p.w);
    size_t tb = p.tmp_bytes;
    if (hipcub::DeviceRadixSort::SortPairs(p.tmp, tb, p.w, p.keyB, a->cls_ord, p.pord, (int)E, 0,
                                           plan_key_bits(NS), st) != hipSuccess)
      return pf::fail(where, "radix sort (plan order)");
    hipLaunchKernelGGL(k_plan_class<true>, dim3((unsigned)NT), dim3(256), 0, st, NF, NC, (int)NT,
                       -1, nullptr, a->cls_ord, a->cls_ptr, a->user_of, a->ci, a->nfields, a->cap,
                       a->visits_in, p.w, a->n_hard, a->completeness, a->cut);
    hipLaunchKernelGGL(k_plan_fiber_csr<false>, dim3((unsigned)((NS + 3) / 4)), dim3(256), 0, st,
                       NS, a->fib_ptr, p.pord, a->tgt_p, a->user_of, p.w, a->ci, a->total_time, o);
  } else {
    const int NFB = (NF + 255) / 256;
    hipLaunchKernelGGL(k_plan_class<false>, dim3((unsigned)NT), dim3(256), 0, st, NF, NC, (int)NT,
                       a->mode, a->perm, nullptr, nullptr, nullptr, a->ci, a->nfields, a->cap,
                       a->visits_in, p.w, a->n_hard, a->completeness, a->cut);
    hipLaunchKernelGGL(k_plan_fiber<false>, dim3((unsigned)(G * NFB)), dim3(256), 0, st, NF, NC,
                       NFB, NS, a->mode, a->perm, p.w, a->ci, a->total_time, o);
  }
  hipLaunchKernelGGL(k_plan_finish, dim3(G), dim3(256), 0, st, NF, NC, a->completeness, a->used,
                     p.ovf, a->utility, a->over, a->worst);
  {
    size_t tb = p.tmp_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(p.tmp, tb, p.cnt, a->seg_ptr, (int)(NS + 1), st) != hipSuccess)
      return pf::fail(where, "scan (segment offsets)");
  }
  if (fill) {
    if (!complete) {
      hipLaunchKernelGGL(k_plan_fiber_csr<true>, dim3((unsigned)((NS + 3) / 4)), dim3(256), 0, st,
                         NS, a->fib_ptr, p.pord, a->tgt_p, a->user_of, p.w, a->ci, a->total_time, o);
    } else {
      const int NFB = (NF + 255) / 256;
      hipLaunchKernelGGL(k_plan_fiber<true>, dim3((unsigned)(G * NFB)), dim3(256), 0, st, NF, NC,
                         NFB, NS, a->mode, a->perm, p.w, a->ci, a->total_time, o);
    }
  }
  return pf::check_launch(where);
}
