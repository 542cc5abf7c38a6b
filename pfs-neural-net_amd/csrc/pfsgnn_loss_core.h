// pfsgnn_loss_core.h -- the training objective's per-edge arithmetic and its
// class reduction / finalize kernels, shared by the complete-graph loss kernels
// (pfsgnn_loss.hip) and the sliced general-graph ones (pfsgnn_sl_loss.hip):
// both translation units compile the same decoder + softplus + softfloor code,
// the LOSS_FAST switch included.
#pragma once
#include "pfsgnn_common.h"
#include "../../include/pfsgnn.h"

#include <cmath>
#include <cstdlib>

__device__ __forceinline__ void wave_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

struct SoftFloor {
  float r, corr, two_pi, inv_pi;  // r = exp(-1/sharpness) (0 if sharpness == 0)
};

static SoftFloor make_softfloor(float sharpness) {
  SoftFloor s;
  const float pi = (float)M_PI;                           // x.new_tensor(np.pi)
  s.r = sharpness == 0.f ? 0.f : expf(-1.0f / sharpness); // train.py:26
  s.corr = atanf(s.r / (1.0f - s.r));
  s.two_pi = 2.0f * pi;
  s.inv_pi = 1.0f / pi;
  return s;
}

// The record from a DEVICE sharpness (a captured step anneals it per replay,
// train.py:137): r = exp(-1/s) and corr = atan(r / (1 - r)) in double, each
// rounded once to float.  s == 0 gives r = corr = 0 exactly (train.py:26); a
// tiny s underflows to the same (exp(-2000) = 0 in double), never NaN.  One
// thread calls it (k_softfloor_record, k_train_advance: pfsgnn_train.hip); the
// loss kernels read the record through their sf_dev pointer.
__device__ __forceinline__ void softfloor_fill(float sharpness, SoftFloor* out) {
  const double s = (double)sharpness;
  const double r = s == 0.0 ? 0.0 : exp(-1.0 / s);
  const float pi = (float)M_PI;
  out->r = (float)r;
  out->corr = (float)atan(r / (1.0 - r));
  out->two_pi = 2.0f * pi;
  out->inv_pi = 1.0f / pi;
}

// the loss ops on a sliced general batch (pfsgnn_sl_loss.hip), reached from
// pfsgnn_loss_fwd / pfsgnn_loss_bwd (pfsgnn_loss.hip) when a->sl is set
int pf_sl_loss_fwd(const pfsgnn_loss_args& a, void* ws, size_t ws_bytes, void* stream);
int pf_sl_loss_bwd(const pfsgnn_loss_args& a, void* ws, size_t ws_bytes, void* stream);

// both backwards' per-block partials pW [nb][F][F+1] (dWd1 | dbd1) and pV
// [nb][F+1] (dWd2 | dbd2) summed into the decoder's gradients, one launch
static void loss_bwd_reduce(const pfsgnn_loss_args& a, float* pW, float* pV, size_t nb,
                            hipStream_t st) {
  const int F = a.F;
  const RedDesc rd[4] = {{pW, (int)nb, (size_t)F * (F + 1), F + 1, F, F, a.dWd1, F, 1, 1.f},
                         {pW + F, (int)nb, (size_t)F * (F + 1), F + 1, F, 1, a.dbd1, 1, 1, 1.f},
                         {pV, (int)nb, (size_t)(F + 1), F, 1, F, a.dWd2, F, 1, 1.f},
                         {pV + F, (int)nb, (size_t)(F + 1), 1, 1, 1, a.dbd2, 1, 1, 1.f}};
  launch_reduce_multi(rd, 4, st);
}

// decoder_e + softplus*scale + softfloor + clamp (train.py:42-49, gnn.py:307-312).
// LOSS_FAST: sin / cos of 2 pi x as one sincospi of 2x (the reduction is exact
// in revolutions, no large-argument path) and one reciprocal of T_i per edge
// for the two divisions by it
#ifndef LOSS_FAST
#define LOSS_FAST 1
#endif
template <int F>
struct EdgeLoss {
  float zd[F], ad[F], pred, time, Ti, xx, th, graw, gal, tt, cth, invTi;
  __device__ __forceinline__ void run(const float (&x)[F], const float* __restrict__ Wd1,
                                      const float* __restrict__ bd1, const float* __restrict__ Wd2,
                                      const float* __restrict__ bd2, float scale, float Ti_,
                                      float noise, const SoftFloor& sf) {
    pred = bd2[0];
#pragma unroll
    for (int j = 0; j < F; ++j) {
      float s = bd1[j];
#pragma unroll
      for (int k = 0; k < F; ++k) s = fmaf(Wd1[j * F + k], x[k], s);
      zd[j] = s;
      ad[j] = lrelu(s);
      pred = fmaf(Wd2[j], ad[j], pred);
    }
    const float sp = pred > 20.f ? pred : log1pf(expf(pred));  // F.softplus (threshold 20)
    time = sp * scale;
    Ti = Ti_;
#if LOSS_FAST
    invTi = 1.0f / Ti;
    xx = fmaf(time, invTi, noise);
    float sth;
    sincospif(2.0f * xx, &sth, &cth);
    graw = xx + sf.inv_pi * (atanf(sf.r * sth / (1.0f - sf.r * cth)) - sf.corr);
#else
    xx = time / Ti + noise;
    th = sf.two_pi * xx;
    cth = cosf(th);
    graw = xx + sf.inv_pi * (atanf(sf.r * sinf(th) / (1.0f - sf.r * cth)) - sf.corr);
#endif
    gal = graw < 0.f ? 0.f : graw;  // torch.maximum(0, g) (NaN propagates)
    tt = gal * Ti;
  }
};

// EdgeLoss<F>::run up to `time` alone -- decoder_e and softplus * scale in the
// same FMA order, without softfloor's trigonometry: what the hard schedule
// (pfsgnn_schedule.hip) floors or rounds
template <int F>
struct EdgeTime {
  float pred, time;
  __device__ __forceinline__ void run(const float (&x)[F], const float* __restrict__ Wd1,
                                      const float* __restrict__ bd1, const float* __restrict__ Wd2,
                                      const float* __restrict__ bd2, float scale) {
    pred = bd2[0];
#pragma unroll
    for (int j = 0; j < F; ++j) {
      float s = bd1[j];
#pragma unroll
      for (int k = 0; k < F; ++k) s = fmaf(Wd1[j * F + k], x[k], s);
      pred = fmaf(Wd2[j], lrelu(s), pred);
    }
    const float sp = pred > 20.f ? pred : log1pf(expf(pred));  // F.softplus (threshold 20)
    time = sp * scale;
  }
};

// decoder_e's weights staged in LDS (read as broadcasts inside the edge loop):
// held in SGPRs they overflowed the scalar file (119 / 139 SGPR spills, each
// use a v_readlane in the loop)
template <int F>
struct DecW {
  static constexpr int N = F * F + 2 * F + 1;
  float w[N];   // Wd1 [F][F] | bd1 [F] | Wd2 [F] | bd2
  __device__ __forceinline__ void load(const float* __restrict__ Wd1, const float* __restrict__ bd1,
                                       const float* __restrict__ Wd2, const float* __restrict__ bd2) {
    for (int i = threadIdx.x; i < N; i += blockDim.x)
      w[i] = i < F * F ? Wd1[i] : i < F * F + F ? bd1[i - F * F]
                                : i < F * F + 2 * F ? Wd2[i - F * F - F] : bd2[0];
  }
};
// the weights' base as an opaque value per loop iteration: the compiler would
// otherwise hoist all F*F + 2F + 1 loop-invariant reads into VGPRs (occupancy 7 -> 3)
template <int F>
__device__ __forceinline__ const float* dec_base(const DecW<F>& d) {
  int lo = 0;
  asm volatile("" : "+v"(lo));
  return d.w + lo;
}
// EdgeTime on the staged weights (DecW's layout: Wd1 | bd1 | Wd2 | bd2)
template <int F>
__device__ __forceinline__ float edge_time(const float (&x)[F], const DecW<F>& dw, float scale) {
  EdgeTime<F> L;
  const float* dwp = dec_base(dw);
  L.run(x, dwp, dwp + F * F, dwp + F * F + F, dwp + F * F + 2 * F, scale);
  return L.time;
}

// ---- the dense loss kernels' iteration (pfsgnn_loss.hip, pfsgnn_schedule.hip):
// EdgeGeo's block -> (graph, 64-fiber group, class split), lane = fiber, wave w
// the classes c0 + w, c0 + w + 4, ...
#define EDGE_PROLOGUE                                                       \
  const int t = threadIdx.x, lane = t & 63;                                 \
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);                  \
  const int bx = PF_LOGICAL_BLOCK(geo);                                     \
  if (bx >= geo.nblocks) return;                                            \
  const int ks = bx % geo.KS, grp = bx / geo.KS;                            \
  const int fg = grp % geo.NFG, gg = grp / geo.NFG;                         \
  const int f = fg * 64 + lane;                                             \
  const bool fvalid = f < geo.NF;                                           \
  const long long n = (long long)gg * geo.NF + (fvalid ? f : 0);            \
  const long long nbase = (long long)gg * geo.NF + (long long)fg * 64;      \
  const int nvalid = min(64, geo.NF - fg * 64);                             \
  const int c0 = ks * geo.CPS, c1 = min(geo.NC, c0 + geo.CPS);              \
  const long long E = geo.E, NS = geo.NS, NT = geo.NT;                      \
  (void)E; (void)NS; (void)NT; (void)n; (void)nbase; (void)nvalid; (void)t;

#define CLASS_LOOP_BEGIN                                                    \
  for (int c = c0 + wave; c < c1; c += 4) {                                 \
    const long long cn = (long long)gg * geo.NC + c;                        \
    const long long e = cn * geo.NF + (fvalid ? f : 0);                     \
    const long long eu = n * geo.NC + c; /* train.py's fiber-major position */

#define CLASS_LOOP_END }

// the next class's edge rows of this wave prefetched one iteration ahead
// (register ring; the loop body is one long dependent chain per class)
#define Y_PREFETCH_DECL(F)                                                    \
  float yq[F];                                                              \
  auto yload = [&](int cc) {                                                \
    const long long ee = ((long long)gg * geo.NC + cc) * geo.NF + (fvalid ? f : 0); \
    _Pragma("unroll") for (int k = 0; k < F; ++k)                           \
      yq[k] = (fvalid && cc < c1) ? y[(long long)k * E + ee] : 0.f;         \
  };                                                                        \
  yload(c0 + wave);
#define Y_TAKE(F, x)                                                          \
  _Pragma("unroll") for (int k = 0; k < F; ++k)                             \
    x[k] = sc ? fmaf(yq[k], sc[k], sh[k]) : yq[k];                          \
  yload(c + 4);

// Canonical index k = (g*NC + c)*NF + f.  mode 0: user edge id = perm[k];
// mode 1: user order is train.py's fiber-major (g*NF + f)*NC + c (graph.py /
// cartesian_prod, train.py:94); mode 2: user order is already canonical.
__device__ __forceinline__ long long user_index(long long k, int NF, int NC, int mode,
                                                const int32_t* __restrict__ perm) {
  if (mode == 2) return k;
  if (mode == 0) return perm[k];
  const long long gc = k / NF, f = k - gc * NF;
  const long long g = gc / NC, c = gc - g * NC;
  return (g * NF + f) * NC + c;
}
// the same for a kernel that walks (g, c, f) and has the fiber-major index at
// hand: no divisions.  (user_index is not built on it: its early returns
// compile to other code in k_to_canonical / k_from_canonical than a select)
__device__ __forceinline__ long long caller_pos(int mode, long long k, long long fiber_major,
                                                const int32_t* __restrict__ perm) {
  return mode == 2 ? k : (mode == 1 ? fiber_major : (long long)perm[k]);
}


// the loss kernels' grid: class splits to about PFSGNN_LOSS_BLOCKS blocks
// (A/B knob; default PF_TARGET_BLOCKS)
inline EdgeGeo loss_geo(int G, int NF, int NC) {
  static const int tb = [] {
    const char* e = getenv("PFSGNN_LOSS_BLOCKS");
    return e && atoi(e) > 0 ? atoi(e) : PF_TARGET_BLOCKS;
  }();
  return make_geo(G, NF, NC, tb);
}

// ---- the sliced loss kernels' iteration (pfsgnn_sl_loss.hip, pfsgnn_schedule.hip;
// `sl` a pfm::SlGeo, `geo` pfm::sl_geo's): a lane owns an edge, four steps per
// iteration
#define SLL_PROLOGUE                                                                   \
  const int t = threadIdx.x, lane = t & 63;                                            \
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);                             \
  const int q4 = lane >> 4, j16 = lane & 15;                                           \
  const int bx = blockIdx.x;                                                           \
  const int ks = bx % geo.KS, grp = bx / geo.KS;                                       \
  const int gg = grp / geo.NFG;                                                        \
  const int slc = 4 * grp + wave;                                                      \
  const int fib = sl.fib[slc * 16 + j16];   /* global fiber of the lane, -1: none */   \
  const int pb = __builtin_amdgcn_readfirstlane(sl.base[slc]);                         \
  const int Ls = __builtin_amdgcn_readfirstlane(sl.len[slc]);                          \
  /* split ks of KS: steps [k0, k1) of the slice, four per iteration */                \
  const int k0 = (int)(((long long)Ls * ks) / geo.KS);                                 \
  const int k1 = (int)(((long long)Ls * (ks + 1)) / geo.KS);                           \
  const int nit = (k1 - k0 + 3) >> 2;                                                  \
  const int NC = geo.NC;                                                               \
  const long long EP = geo.E, NS = geo.NS;                                             \
  const long long cn0 = (long long)gg * NC;                                            \
  const long long p0 = (long long)pb + 16ll * k0 + lane;                               \
  (void)NS; (void)t; (void)nit; (void)EP; (void)cn0;

// the lane's edge of one iteration: channel rows, class byte, caller edge id
// (steps beyond the split load nothing: class 0xFF, edge -1, rows 0)
template <int F>
struct SlEdge {
  float y[F];
  int cls, pos;
  bool in;   // the step belongs to this block's split (its position is ours to write)
};
#define SLL_LOAD_DECL(F)                                                               \
  auto load = [&](int i) {                                                             \
    SlEdge<F> r;                                                                       \
    r.in = k0 + 4 * i + q4 < k1;                                                       \
    const long long p = p0 + 64ll * i;                                                 \
    r.cls = r.in ? (int)sl.cls[p] : 0xFF;                                              \
    r.pos = r.in ? pos_user[p] : -1;                                                   \
    _Pragma("unroll") for (int k = 0; k < F; ++k)                                      \
      r.y[k] = r.in ? y[(long long)k * EP + p] : 0.f;                                  \
    return r;                                                                          \
  };
// the same with the position opaque per iteration, and the rows addressed from
// it: the compiler would otherwise keep one 64-bit row address per channel
// across the loop (2 F VGPRs).  pfsgnn_schedule.hip's time pass uses it
#define SLL_LOAD_OPAQUE_DECL(F)                                                        \
  auto load = [&](int i) {                                                             \
    SlEdge<F> r;                                                                       \
    r.in = k0 + 4 * i + q4 < k1;                                                       \
    long long p = p0 + 64ll * i;                                                       \
    asm volatile("" : "+v"(p));                                                        \
    r.cls = r.in ? (int)sl.cls[p] : 0xFF;                                              \
    r.pos = r.in ? pos_user[p] : -1;                                                   \
    const float* yp = y + p;                                                           \
    _Pragma("unroll") for (int k = 0; k < F; ++k)                                      \
      r.y[k] = r.in ? yp[(long long)k * EP] : 0.f;                                     \
    return r;                                                                          \
  };
// validity and the class clamped to 0 (padding 0xFF, steps beyond the split and
// lanes without a fiber never index a class table with their raw byte)
#define SLL_STEP(e)                                                                    \
  const bool ev = (e).in && fib >= 0 && (e).cls < NC && (e).pos >= 0;                  \
  const int cl = ev ? (e).cls : 0;                                                     \
  const long long cn = cn0 + cl;

__device__ __forceinline__ double wave_dsum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// one wave per class: lane l takes the fiber groups l, l + 64, ... and the
// moments merge in closed form (mean = sum c_b m_b / sum c_b, M2 = sum (q_b +
// c_b (m_b - mean)^2), in double; fixed lane and butterfly order): the loads
// are independent, where a per-thread Chan chain ran NFG dependent divisions.
// RAGGED (a general batch: every class has its own edge count, the partials'
// counts summed): the unbiased variance over the class's own deg(c) edges, 0
// when deg(c) < 2 (an empty class: n' = 0, tmean = 0, tvar = 0), and deg(c) as
// a second row of tvar ([2][G*NC]) for the finalize
template <bool RAGGED>
__global__ __launch_bounds__(256) void k_loss_class_reduce(const float* __restrict__ part, int G,
                                                           int NFG, int NC, int NF,
                                                           float* __restrict__ n_prime,
                                                           float* __restrict__ tmean,
                                                           float* __restrict__ tvar) {
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;  // over G*NC
  if (idx >= G * NC) return;
  const int g = idx / NC, c = idx - g * NC;
  const float* q0 = part + ((size_t)g * NFG * NC + c) * 4;
  const size_t stride = (size_t)NC * 4;
  double P = 0, C = 0, S = 0;
  for (int b = lane; b < NFG; b += 64) {
    const float* q = q0 + (size_t)b * stride;
    P += q[0];
    C += q[1];
    S += (double)q[1] * (double)q[2];
  }
  P = wave_dsum(P);
  C = wave_dsum(C);
  S = wave_dsum(S);
  const double M = C > 0 ? S / C : 0.0;
  double Q = 0;
  for (int b = lane; b < NFG; b += 64) {
    const float* q = q0 + (size_t)b * stride;
    const double d = (double)q[2] - M;
    Q += (double)q[3] + (double)q[1] * d * d;
  }
  Q = wave_dsum(Q);
  if (lane == 0) {
    n_prime[idx] = (float)P;
    tmean[idx] = (float)M;
    if constexpr (RAGGED) {
      tvar[idx] = C >= 2.0 ? (float)(Q / (C - 1.0)) : 0.f;
      tvar[(size_t)G * NC + idx] = (float)C;
    } else {
      tvar[idx] = NF > 1 ? (float)(Q / (double)(NF - 1)) : NAN;  // torch.var, correction=1
    }
  }
}

// torch.min propagates NaN (train.py:53: a class with N_i = 0 gives 0/0);
// fminf would drop it
__device__ __forceinline__ float nan_min(float a, float b) {
  return (a != a) ? a : ((b != b) ? b : (b < a ? b : a));
}

// one block per graph: train.py:53-71 and the per-node gradient coefficients.
// RAGGED: tvar is k_loss_class_reduce<true>'s [2][NT] (row 1 = deg(c)); the
// variance gradient coefficient of class c is -wvar * 2 / (deg(c) - 1), 0 when
// deg(c) < 2
template <bool RAGGED>
__global__ __launch_bounds__(256) void k_loss_finalize(
    int NF, int NC, int NT, const float* __restrict__ n_prime, const float* __restrict__ fiber_time,
    const float* __restrict__ tvar, const float* __restrict__ ci, float pclass, float pfiber,
    float total_time, float nfields, float wutils, float wvar, float* __restrict__ loss,
    float* __restrict__ utils, float* __restrict__ variance, float* __restrict__ Gn,
    float* __restrict__ Gf, float* __restrict__ Gv) {
  const int g = blockIdx.x, t = threadIdx.x;
  __shared__ float scratch[4 * 4];
  __shared__ float smin[256];
  // completeness min
  float mn = INFINITY;
  for (int c = t; c < NC; c += 256) {
    const long long cn = (long long)g * NC + c;
    const float Ni = ci[NT + cn] / nfields;
    const float comp = n_prime[cn] / Ni;
    mn = nan_min(mn, comp);
  }
  smin[t] = mn;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) smin[t] = nan_min(smin[t], smin[t + s]);
    __syncthreads();
  }
  const float umin = smin[0];
  float v[4] = {0.f, 0.f, 0.f, 0.f};  // ties, class penalty, fiber penalty, variance
  for (int c = t; c < NC; c += 256) {
    const long long cn = (long long)g * NC + c;
    const float Ni = ci[NT + cn] / nfields;
    const float comp = n_prime[cn] / Ni;
    v[0] += comp == umin ? 1.f : 0.f;
    const float over = fmaxf(n_prime[cn] - Ni, 0.f);
    v[1] += over * over;
    v[3] += tvar[cn];
  }
  for (int f = t; f < NF; f += 256) {
    const long long n = (long long)g * NF + f;
    const float ot = fiber_time[n] - total_time;
    const float lk = lrelu(ot);
    v[2] += lk * lk;
    Gf[n] = pfiber * 2.f * lk * dlrelu(ot);
  }
  block_sum<4>(v, scratch);
  const float ties = v[0];
  for (int c = t; c < NC; c += 256) {
    const long long cn = (long long)g * NC + c;
    const float Ni = ci[NT + cn] / nfields;
    const float comp = n_prime[cn] / Ni;
    const float over = fmaxf(n_prime[cn] - Ni, 0.f);
    Gn[cn] = (comp == umin ? -wutils / ties : 0.f) / Ni + 2.f * pclass * over;
    if constexpr (RAGGED) {
      const float deg = tvar[NT + cn];
      Gv[cn] = deg >= 2.f ? -wvar * 2.f / (deg - 1.f) : 0.f;
    } else {
      Gv[cn] = -wvar * 2.f / (float)(NF - 1);
    }
  }
  if (t == 0) {
    utils[g] = umin;
    variance[g] = v[3];
    loss[g] = -wutils * umin + pfiber * v[2] + pclass * v[1] - wvar * v[3];
  }
}

// a bump allocator over the caller's workspace (256-byte aligned pieces)
struct LossWs {
  char* p;
  size_t left;
  float* take(size_t nfloats) {
    const size_t b = align256(nfloats * sizeof(float));
    if (b > left) return nullptr;
    float* r = reinterpret_cast<float*>(p);
    p += b;
    left -= b;
    return r;
  }
};

#define LOSS_DISPATCH_F(F, ...)                              \
  switch (F) {                                               \
    case 8: { constexpr int FF = 8; __VA_ARGS__; } break;    \
    case 10: { constexpr int FF = 10; __VA_ARGS__; } break;  \
    case 16: { constexpr int FF = 16; __VA_ARGS__; } break;  \
    default: return pf::fail("dispatch", "unsupported F");   \
  }
