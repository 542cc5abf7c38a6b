// pfsgnn_loss.hip -- the training objective (train.py:21-80) fused over edges,
// and the edge-layout helpers (canonical order <-> the caller's edge_index).
#include "pfsgnn_common.h"
#include "pfsgnn_loss_core.h"   // the per-edge arithmetic, class reduce and finalize
#include "../../include/pfsgnn.h"

#include <algorithm>
#include <cmath>

template <int F>
__global__ __launch_bounds__(256) void k_loss_fwd(EdgeGeo geo, const float* __restrict__ y,
                                                  const float* __restrict__ sc,
                                                  const float* __restrict__ sh,
                                                  const float* __restrict__ Wd1,
                                                  const float* __restrict__ bd1,
                                                  const float* __restrict__ Wd2,
                                                  const float* __restrict__ bd2,
                                                  const float* __restrict__ ci, float scale,
                                                  SoftFloor sf0,
                                                  const SoftFloor* __restrict__ sf_dev,
                                                  float noiselevel, uint64_t key0,
                                                  const unsigned long long* __restrict__ seed_dev,
                                                  float* __restrict__ fiber_time,
                                                  float* __restrict__ tt_out,
                                                  float* __restrict__ part) {
  EDGE_PROLOGUE
  const uint64_t key = seed_dev ? pf_noise_key(*seed_dev) : key0;
  const SoftFloor sf = sf_dev ? *sf_dev : sf0;   // wave-uniform: scalar loads
  __shared__ float scratch[4 * 64];
  __shared__ __attribute__((aligned(16))) DecW<F> dw;
  dw.load(Wd1, bd1, Wd2, bd2);
  __syncthreads();
  float ft = 0.f;
  const float nw = (float)nvalid;
  Y_PREFETCH_DECL(F)
  CLASS_LOOP_BEGIN
    (void)e;
    float x[F];
    Y_TAKE(F, x)
    const float noise = noiselevel * (pf_uniform(key, (uint64_t)eu) - 0.5f);
    EdgeLoss<F> L;
    const float* dwp = dec_base(dw);
    L.run(x, dwp, dwp + F * F, dwp + F * F + F, dwp + F * F + 2 * F, scale, ci[cn], noise, sf);
    const float tt = fvalid ? L.tt : 0.f;
    ft += tt;
    if (tt_out && fvalid) tt_out[eu] = L.tt;
    const float np = wave_sum(fvalid ? L.gal : 0.f);
    const float mw = wave_sum(tt) / nw;
    const float dv = fvalid ? tt - mw : 0.f;
    const float qw = wave_sum(dv * dv);
    if (lane == 0) {
      float* o = part + (((size_t)gg * geo.NFG + fg) * geo.NC + c) * 4;
      o[0] = np; o[1] = nw; o[2] = mw; o[3] = qw;
    }
  CLASS_LOOP_END
  // fiber time: merge the 4 waves, KS-partial per fiber
  __syncthreads();
  scratch[wave * 64 + lane] = ft;
  __syncthreads();
  if (t < 64 && t < nvalid)
    fiber_time[(size_t)ks * NS + nbase + t] =
        ((scratch[t] + scratch[64 + t]) + scratch[128 + t]) + scratch[192 + t];
}

template <int F, bool BN>
__global__ __launch_bounds__(256) void k_loss_bwd(EdgeGeo geo, const float* __restrict__ y,
                                                  const float* __restrict__ sc,
                                                  const float* __restrict__ sh,
                                                  const float* __restrict__ Wd1,
                                                  const float* __restrict__ bd1,
                                                  const float* __restrict__ Wd2,
                                                  const float* __restrict__ bd2,
                                                  const float* __restrict__ ci, float scale,
                                                  SoftFloor sf0,
                                                  const SoftFloor* __restrict__ sf_dev,
                                                  float noiselevel, uint64_t key0,
                                                  const unsigned long long* __restrict__ seed_dev,
                                                  const float* __restrict__ Gn,
                                                  const float* __restrict__ Gf,
                                                  const float* __restrict__ Gv,
                                                  const float* __restrict__ tmean,
                                                  const float* __restrict__ gscale,
                                                  float* __restrict__ gxe,
                                                  float* __restrict__ partW,
                                                  float* __restrict__ partV,
                                                  const float* __restrict__ bn_mu1,
                                                  const float* __restrict__ bn_inv1,
                                                  float* __restrict__ partBN) {
  using WG = WGrad<F, F + 1>;  // g_zd (x) [x, 1] -> dWd1 | dbd1
  EDGE_PROLOGUE
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
  const float Gf_f = fvalid ? Gf[n] : 0.f;
  // (partBN) the final edge BatchNorm's backward sums of the gradient this
  // kernel writes: sum g and sum g * (y - mu1) * inv1 per channel
  // (1/scale applied once, after the loop)
  float bsg[F], bsx[F];
#pragma unroll
  for (int k = 0; k < F; ++k) bsg[k] = bsx[k] = 0.f;
  Y_PREFETCH_DECL(F)
  CLASS_LOOP_BEGIN
    const float Ti = ci[cn], Gn_c = Gn[cn], Gv_c = Gv[cn], tm_c = tmean[cn];
    float x[F + 1], yr[F];   // (BN: y - mu1, kept for the sums)
#pragma unroll
    for (int k = 0; k < F; ++k) yr[k] = BN ? yq[k] - bn_mu1[k] : 0.f;
    Y_TAKE(F, x)
    x[F] = 1.f;
    const float noise = noiselevel * (pf_uniform(key, (uint64_t)eu) - 0.5f);
    EdgeLoss<F> L;
    float xf[F];
#pragma unroll
    for (int k = 0; k < F; ++k) xf[k] = x[k];
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
    const float g_pred = fvalid ? gs * g_time * scale * sig : 0.f;
    float gz[F];
#pragma unroll
    for (int j = 0; j < F; ++j) {
      acc[j] = fmaf(g_pred, L.ad[j], acc[j]);
      gz[j] = dwp[F * F + F + j] * g_pred * dlrelu(L.zd[j]);
    }
    acc[F] += g_pred;
    if (fvalid) {
#pragma unroll
      for (int k = 0; k < F; ++k) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < F; ++j) s = fmaf(dwp[j * F + k], gz[j], s);
        gxe[(long long)k * E + e] = s;
        if (BN) {
          bsg[k] += s;
          bsx[k] = fmaf(s, yr[k], bsx[k]);
        }
      }
    }
    wg.stage(region, gz, x, lane);
    wave_lds_sync();
    wg.accum(region, lane);
    wave_lds_sync();
  CLASS_LOOP_END
  wg.block_partial(lds, partW + (size_t)bx * F * (F + 1));
  block_sum<F + 1>(acc, lds + LDS_N);
  if (t <= F) {
    float val = 0.f;
#pragma unroll
    for (int i = 0; i <= F; ++i) val = (i == t) ? acc[i] : val;
    partV[(size_t)bx * (F + 1) + t] = val;
  }
  if (BN) {   // [nb][2F]: sum g | sum g xhat, the layout k_bn2_coef_part reads
    __shared__ float bred[4 * 2 * F];
    float v[2 * F];
#pragma unroll
    for (int k = 0; k < F; ++k) {
      v[k] = bsg[k];
      v[F + k] = bsx[k] * bn_inv1[k];
    }
    block_sum<2 * F>(v, bred);
    if (t < 2 * F) {
      float val = 0.f;
#pragma unroll
      for (int i = 0; i < 2 * F; ++i) val = (i == t) ? v[i] : val;
      partBN[(size_t)bx * 2 * F + t] = val;
    }
  }
}

// ------------------------------------------------------------ layout
// (canonical index <-> the caller's edge: user_index, pfsgnn_loss_core.h)
__global__ void k_layout_init(int32_t* status) {
  if (threadIdx.x == 0) { status[0] = 1; status[1] = 1; status[2] = 1; }
}

__global__ void k_layout_scatter(const int64_t* __restrict__ ei, long long E, int G, int NF, int NC,
                                 int32_t* __restrict__ perm, int32_t* __restrict__ cnt,
                                 int32_t* __restrict__ status) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const long long NS = (long long)G * NF, NT = (long long)G * NC;
  const long long s = ei[e], tg = ei[E + e];
  if (s < 0 || s >= NS || tg < 0 || tg >= NT) {
    atomicAnd(&status[0], 0); atomicAnd(&status[1], 0); atomicAnd(&status[2], 0);
    return;
  }
  const long long g = s / NF, gt = tg / NC;
  if (g != gt) {
    atomicAnd(&status[0], 0); atomicAnd(&status[1], 0); atomicAnd(&status[2], 0);
    return;
  }
  const long long f = s - g * NF, c = tg - gt * NC;
  const long long k = (g * NC + c) * NF + f;
  atomicAdd(&cnt[k], 1);
  perm[k] = (int32_t)e;
  if (e != s * NC + c) atomicAnd(&status[1], 0);
  if (e != k) atomicAnd(&status[2], 0);
}

__global__ void k_layout_check(const int32_t* __restrict__ cnt, long long E,
                               int32_t* __restrict__ status) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= E) return;
  if (cnt[k] != 1) { atomicAnd(&status[0], 0); atomicAnd(&status[1], 0); atomicAnd(&status[2], 0); }
}

__global__ void k_to_canonical(const float* __restrict__ src, long long E, int NF, int NC, int F,
                               int mode, const int32_t* __restrict__ perm,
                               float* __restrict__ dst) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= E) return;
  const long long eu = user_index(k, NF, NC, mode, perm);
  for (int j = 0; j < F; ++j) dst[(long long)j * E + k] = src[eu * F + j];
}

__global__ void k_from_canonical(const float* __restrict__ y, const float* __restrict__ sc,
                                 const float* __restrict__ sh, long long E, int NF, int NC, int F,
                                 int mode, const int32_t* __restrict__ perm, int rowmajor,
                                 float* __restrict__ dst) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= E) return;
  const long long eu = user_index(k, NF, NC, mode, perm);
  for (int j = 0; j < F; ++j) {
    float v = y[(long long)j * E + k];
    if (sc) v = fmaf(v, sc[j], sh[j]);
    if (rowmajor) dst[eu * F + j] = v;
    else dst[(long long)j * E + eu] = v;
  }
}

// Fiber-major row-major output (train.py's order) through an LDS tile: a block
// takes 64 fibers x 16 classes of one graph, reads the canonical rows
// coalesced along the fibers, and writes each fiber's 16 classes x F values as
// one contiguous run (dst row (g*NF + f)*NC + c).
#define FC_CT 16
template <int F>
__global__ __launch_bounds__(256) void k_from_canonical_fm(const float* __restrict__ y,
                                                           const float* __restrict__ sc,
                                                           const float* __restrict__ sh, int G,
                                                           int NF, int NC,
                                                           float* __restrict__ dst) {
  __shared__ float tile[64 * FC_CT * F + 64];
  const int t = threadIdx.x;
  const int nfg = (NF + 63) / 64, ncg = (NC + FC_CT - 1) / FC_CT;
  const int b = blockIdx.x;
  const int cg = b % ncg, fg = (b / ncg) % nfg, g = b / (ncg * nfg);
  const int f0 = fg * 64, cb = cg * FC_CT;
  const int nf = min(64, NF - f0), nc = min(FC_CT, NC - cb);
  const long long E = (long long)G * NF * NC;
  // tile[(fl * FC_CT + cl) * F + j]  (fiber-major, then class, then feature)
  for (int idx = t; idx < F * FC_CT * 64; idx += 256) {
    const int fl = idx & 63, rest = idx >> 6;
    const int cl = rest % FC_CT, j = rest / FC_CT;
    if (fl < nf && cl < nc) {
      float v = y[(long long)j * E + ((long long)g * NC + cb + cl) * NF + f0 + fl];
      if (sc) v = fmaf(v, sc[j], sh[j]);
      tile[(fl * FC_CT + cl) * F + j] = v;
    }
  }
  __syncthreads();
  const int run = nc * F;  // contiguous floats per fiber
  for (int idx = t; idx < nf * run; idx += 256) {
    const int fl = idx / run, r = idx - fl * run;
    dst[(((long long)g * NF + f0 + fl) * NC + cb) * F + r] = tile[fl * FC_CT * F + r];
  }
}

__global__ void k_fiber_partial_sum(const float* __restrict__ part, int KS, long long len,
                                    float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= len) return;
  float s = 0.f;
  for (int k = 0; k < KS; ++k) s += part[(size_t)k * len + idx];
  out[idx] = s;
}

// ------------------------------------------------------------ host side
namespace {
using Ws = LossWs;
#define DISPATCH_F LOSS_DISPATCH_F
int check_dims(const char* where, int G, int NF, int NC, int F) {
  if (G <= 0 || NF <= 1 || NC <= 0) return pf::fail(where, "need G > 0, NF > 1, NC > 0");
  if (NC > 256) return pf::fail(where, "NC > 256 is not supported by the dense edge kernels");
  if (F != 8 && F != 10 && F != 16) return pf::fail(where, "unsupported Fdim (8, 10, 16)");
  return 0;
}
}  // namespace


// The loss ops take one argument struct (pfsgnn_loss_args, include/pfsgnn.h);
// a->sl selects the sliced general-graph form (pfsgnn_sl_loss.hip).
static int loss_fwd_dense(const pfsgnn_loss_args& a, void* ws, size_t ws_bytes, void* stream) {
  const char* where = "pfsgnn_loss_fwd";
  const int G = a.G, NF = a.NF, NC = a.NC, F = a.F;
  if (int rc = check_dims(where, G, NF, NC, F)) return rc;
  PF_REQUIRE(a.y && a.Wd1 && a.bd1 && a.Wd2 && a.bd2 && a.ci && a.n_prime && a.fiber_time &&
                 a.tmean && a.tvar,
             where, "null");
  const EdgeGeo geo = loss_geo(G, NF, NC);
  Ws w{reinterpret_cast<char*>(ws), ws_bytes};
  float* part = w.take((size_t)G * geo.NFG * NC * 4);
  float* ftp = geo.KS == 1 ? a.fiber_time : w.take((size_t)geo.KS * geo.NS);
  PF_REQUIRE(part && ftp, where, "workspace too small");
  hipStream_t st = as_stream(stream);
  const SoftFloor sf = make_softfloor(a.sharpness);
  const SoftFloor* sfd = reinterpret_cast<const SoftFloor*>(a.sf_dev);
  const uint64_t key = pf_noise_key((uint64_t)a.seed);
  { pf::Timer tm_("loss_fwd", st);
  DISPATCH_F(F, hipLaunchKernelGGL(k_loss_fwd<FF>, dim3(edge_grid(geo)), dim3(256), 0, st, geo, a.y,
                                   a.sc, a.sh, a.Wd1, a.bd1, a.Wd2, a.bd2, a.ci, a.scale, sf, sfd,
                                   a.noiselevel, key, a.seed_dev, ftp, a.tt, part));
  tm_.end(); }
  if (geo.KS > 1)
    hipLaunchKernelGGL(k_fiber_partial_sum, dim3((unsigned)((geo.NS + 255) / 256)), dim3(256), 0,
                       st, ftp, geo.KS, geo.NS, a.fiber_time);
  hipLaunchKernelGGL(k_loss_class_reduce<false>, dim3((G * NC + 3) / 4), dim3(256), 0, st, part, G,
                     geo.NFG, NC, NF, a.n_prime, a.tmean, a.tvar);
  return pf::check_launch(where);
}

// what every form of the struct must satisfy, before any launch
static int loss_args_check(const char* where, const pfsgnn_loss_args* a) {
  PF_REQUIRE(a, where, "null argument struct");
  PF_REQUIRE(!a->sl == !a->pos_user, where,
             "sl and pos_user go together (both set: a sliced general batch; both NULL: complete)");
  const int nbn = (a->bn_mu1 != nullptr) + (a->bn_inv1 != nullptr) + (a->bn_part != nullptr);
  PF_REQUIRE(nbn == 0 || nbn == 3, where, "bn_mu1, bn_inv1 and bn_part go together");
  PF_REQUIRE(!(a->sl && nbn), where,
             "sl with bn_part: the final BatchNorm's sums are not fused on a sliced batch");
  return 0;
}

extern "C" size_t pfsgnn_loss_args_bytes(void) { return sizeof(pfsgnn_loss_args); }

extern "C" int pfsgnn_loss_fwd(const pfsgnn_loss_args* a, void* ws, size_t ws_bytes,
                               void* stream) {
  if (int rc = loss_args_check("pfsgnn_loss_fwd", a)) return rc;
  return a->sl ? pf_sl_loss_fwd(*a, ws, ws_bytes, stream) : loss_fwd_dense(*a, ws, ws_bytes, stream);
}

extern "C" int pfsgnn_loss_finalize(const pfsgnn_sliced_t* sl, int G, int NF, int NC,
                                    const float* n_prime, const float* fiber_time,
                                    const float* tvar, const float* ci, float pclass, float pfiber,
                                    float total_time, float nfields, float wutils, float wvar,
                                    float* loss, float* utils, float* variance, float* Gn,
                                    float* Gf, float* Gv, void* stream) {
  PF_REQUIRE(G > 0 && NF > 1 && NC > 0, "pfsgnn_loss_finalize", "bad dims");
  PF_REQUIRE(n_prime && fiber_time && tvar && ci && loss && utils && variance && Gn && Gf && Gv,
             "pfsgnn_loss_finalize", "null");
  // a sliced batch: tvar is [2][NT], its second row the class edge counts
  const auto kern = sl ? k_loss_finalize<true> : k_loss_finalize<false>;
  hipLaunchKernelGGL(kern, dim3(G), dim3(256), 0, as_stream(stream), NF, NC, G * NC, n_prime,
                     fiber_time, tvar, ci, pclass, pfiber, total_time, nfields, wutils, wvar, loss,
                     utils, variance, Gn, Gf, Gv);
  return pf::check_launch("pfsgnn_loss_finalize");
}

static int loss_bwd_dense(const pfsgnn_loss_args& a, void* ws, size_t ws_bytes, void* stream) {
  const char* where = "pfsgnn_loss_bwd";
  const int G = a.G, NF = a.NF, NC = a.NC, F = a.F;
  if (int rc = check_dims(where, G, NF, NC, F)) return rc;
  PF_REQUIRE(a.y && a.Wd1 && a.bd1 && a.Wd2 && a.bd2 && a.ci && a.Gn && a.Gf && a.Gv && a.tmean &&
                 a.dWd1 && a.dbd1 && a.dWd2 && a.dbd2 && a.gxe,
             where, "null");
  const EdgeGeo geo = loss_geo(G, NF, NC);
  const size_t nb = geo.nblocks;
  Ws w{reinterpret_cast<char*>(ws), ws_bytes};
  float* pW = w.take(nb * F * (F + 1));
  float* pV = w.take(nb * (F + 1));
  PF_REQUIRE(pW && pV, where, "workspace too small");
  hipStream_t st = as_stream(stream);
  const SoftFloor sf = make_softfloor(a.sharpness);
  const SoftFloor* sfd = reinterpret_cast<const SoftFloor*>(a.sf_dev);
  const uint64_t key = pf_noise_key((uint64_t)a.seed);
  { pf::Timer tm_("loss_bwd", st);
  if (a.bn_part) {
    DISPATCH_F(F, hipLaunchKernelGGL((k_loss_bwd<FF, true>), dim3(edge_grid(geo)), dim3(256), 0, st,
                                     geo, a.y, a.sc, a.sh, a.Wd1, a.bd1, a.Wd2, a.bd2, a.ci, a.scale,
                                     sf, sfd, a.noiselevel, key, a.seed_dev, a.Gn, a.Gf, a.Gv,
                                     a.tmean, a.gscale, a.gxe, pW, pV, a.bn_mu1, a.bn_inv1,
                                     a.bn_part));
  } else {
    DISPATCH_F(F, hipLaunchKernelGGL((k_loss_bwd<FF, false>), dim3(edge_grid(geo)), dim3(256), 0, st,
                                     geo, a.y, a.sc, a.sh, a.Wd1, a.bd1, a.Wd2, a.bd2, a.ci, a.scale,
                                     sf, sfd, a.noiselevel, key, a.seed_dev, a.Gn, a.Gf, a.Gv,
                                     a.tmean, a.gscale, a.gxe, pW, pV, nullptr, nullptr, nullptr));
  }
  tm_.end(); }
  loss_bwd_reduce(a, pW, pV, nb, st);
  return pf::check_launch(where);
}

extern "C" int pfsgnn_loss_bwd(const pfsgnn_loss_args* a, void* ws, size_t ws_bytes,
                               void* stream) {
  if (int rc = loss_args_check("pfsgnn_loss_bwd", a)) return rc;
  return a->sl ? pf_sl_loss_bwd(*a, ws, ws_bytes, stream) : loss_bwd_dense(*a, ws, ws_bytes, stream);
}

extern "C" int pfsgnn_loss_bn_parts(int G, int NF, int NC) {
  return loss_geo(G, NF, NC).nblocks;
}

extern "C" int pfsgnn_layout_analyze(const int64_t* edge_index, long long E, int G, int NF, int NC,
                                     int32_t* perm, int32_t* status, void* ws, size_t ws_bytes,
                                     void* stream) {
  PF_REQUIRE(edge_index && perm && status && E > 0, "pfsgnn_layout_analyze", "null/empty");
  PF_REQUIRE(E == (long long)G * NF * NC, "pfsgnn_layout_analyze",
             "E != G*NF*NC: not a complete bipartite batch");
  PF_REQUIRE(E < (1ll << 31), "pfsgnn_layout_analyze", "E too large for int32 permutation");
  PF_REQUIRE(ws && ws_bytes >= (size_t)E * sizeof(int32_t), "pfsgnn_layout_analyze",
             "workspace too small");
  hipStream_t st = as_stream(stream);
  int32_t* cnt = reinterpret_cast<int32_t*>(ws);
  if (hipMemsetAsync(cnt, 0, (size_t)E * sizeof(int32_t), st) != hipSuccess)
    return pf::fail("pfsgnn_layout_analyze", "memset");
  hipLaunchKernelGGL(k_layout_init, dim3(1), dim3(64), 0, st, status);
  const unsigned nbk = (unsigned)((E + 255) / 256);
  hipLaunchKernelGGL(k_layout_scatter, dim3(nbk), dim3(256), 0, st, edge_index, E, G, NF, NC, perm,
                     cnt, status);
  hipLaunchKernelGGL(k_layout_check, dim3(nbk), dim3(256), 0, st, cnt, E, status);
  return pf::check_launch("pfsgnn_layout_analyze");
}

extern "C" int pfsgnn_edges_to_canonical(const float* src, int G, int NF, int NC, int F, int mode,
                                         const int32_t* perm, float* dst, void* stream) {
  const long long E = (long long)G * NF * NC;
  PF_REQUIRE(src && dst && E > 0 && F > 0 && mode >= 0 && mode <= 2 && (mode != 0 || perm),
             "pfsgnn_edges_to_canonical", "bad arguments");
  hipLaunchKernelGGL(k_to_canonical, dim3((unsigned)((E + 255) / 256)), dim3(256), 0,
                     as_stream(stream), src, E, NF, NC, F, mode, perm, dst);
  return pf::check_launch("pfsgnn_edges_to_canonical");
}

extern "C" int pfsgnn_edges_from_canonical(const float* y, const float* sc, const float* sh, int G,
                                           int NF, int NC, int F, int mode, const int32_t* perm,
                                           int rowmajor, float* dst, void* stream) {
  const long long E = (long long)G * NF * NC;
  PF_REQUIRE(y && dst && E > 0 && F > 0 && mode >= 0 && mode <= 2 && (mode != 0 || perm),
             "pfsgnn_edges_from_canonical", "bad arguments");
  if (mode == 1 && rowmajor && (F == 8 || F == 10 || F == 16)) {
    const unsigned nb = (unsigned)((long long)G * ((NF + 63) / 64) * ((NC + FC_CT - 1) / FC_CT));
    switch (F) {
      case 8: hipLaunchKernelGGL(k_from_canonical_fm<8>, dim3(nb), dim3(256), 0,
                                 as_stream(stream), y, sc, sh, G, NF, NC, dst); break;
      case 10: hipLaunchKernelGGL(k_from_canonical_fm<10>, dim3(nb), dim3(256), 0,
                                  as_stream(stream), y, sc, sh, G, NF, NC, dst); break;
      default: hipLaunchKernelGGL(k_from_canonical_fm<16>, dim3(nb), dim3(256), 0,
                                  as_stream(stream), y, sc, sh, G, NF, NC, dst); break;
    }
    return pf::check_launch("pfsgnn_edges_from_canonical");
  }
  hipLaunchKernelGGL(k_from_canonical, dim3((unsigned)((E + 255) / 256)), dim3(256), 0,
                     as_stream(stream), y, sc, sh, E, NF, NC, F, mode, perm, rowmajor, dst);
  return pf::check_launch("pfsgnn_edges_from_canonical");
}
