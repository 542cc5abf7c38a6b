// pfsgnn_train.hip -- the training loop's per-epoch bookkeeping on the device
// (train.py:133-165): the epoch / seed / sharpness schedule, the history rows
// and best-tracking, and the conditional snapshot of the best state.  With
// these a whole epoch is one captured graph: no host value enters a replay.
// Plain C++, vector stores, no atomics; nothing allocates or synchronises.
#include "pfsgnn_common.h"
#include "pfsgnn_loss_core.h"   // SoftFloor, softfloor_fill
#include "../../include/pfsgnn.h"

#include <cstdint>

__global__ void k_softfloor_record(const float* __restrict__ sharpness, SoftFloor* __restrict__ sf) {
  if (blockIdx.x == 0 && threadIdx.x == 0) softfloor_fill(sharpness[0], sf);
}

// train.py:137 in double, in the expression's own order (no contraction: the
// product, the quotient and the sum each round once), rounded once to float
__global__ void k_train_advance(long long* __restrict__ epoch,
                                unsigned long long* __restrict__ seed, double s0, double s1,
                                long long nepochs, float* __restrict__ sharpness,
                                SoftFloor* __restrict__ sf) {
#pragma clang fp contract(off)
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const long long e = epoch[0] + 1;
  epoch[0] = e;
  seed[0] = seed[0] + 1ull;
  const double prod = (s1 - s0) * (double)e;
  const double quot = prod / (double)nepochs;
  const float s = (float)(s0 + quot);
  sharpness[0] = s;
  softfloor_fill(s, sf);
}

// one block; thread 0 owns the scalars, every thread the completion row
__global__ __launch_bounds__(256) void k_train_record(pfsgnn_train_record_args a) {
  const int t = threadIdx.x;
  const long long NT = (long long)a.G * a.NC;
  const long long e = a.epoch[0];
  const bool hist = e >= 0 && e < a.nepochs;
  for (long long c = t; c < NT; c += 256) {
    const float Ni = a.ci[NT + c] / a.nfields;      // train.py:53
    const float comp = a.n_prime[c] / Ni;
    a.comp[c] = comp;
    if (a.completions && hist) a.completions[c * a.nepochs + e] = comp;
  }
  if (t != 0) return;
  float loss = a.loss[0], util = a.utils[0], var = a.variance[0];
  for (int g = 1; g < a.G; ++g) {
    loss += a.loss[g];
    util += a.utils[g];
    var += a.variance[g];
  }
  if (hist) {
    a.losses[e] = loss;
    a.objective[e] = util;
    a.variances[e] = var;
  }
  // train.py:146 (a NaN utility compares false)
  const bool improved = util > a.best_utility[0] && a.sharpness[0] > a.min_sharp;
  a.improved[0] = improved ? 1 : 0;
  if (improved) {
    a.best_utility[0] = util;
    a.best_loss[0] = loss;
    a.best_epoch[0] = e;
  }
}

// the integer objective's history rows and best-tracking (after
// pfsgnn_schedule): one thread
__global__ void k_train_record_hard(pfsgnn_train_record_hard_args a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const long long e = a.epoch[0];
  float util = a.utility[0];
  int over = a.over[0];
  for (int g = 1; g < a.G; ++g) {
    util += a.utility[g];
    over += a.over[g];
  }
  if (e >= 0 && e < a.nepochs) {
    a.hard_objective[e] = util;
    a.hard_overtime[e] = over;
  }
  const bool improved = util > a.best_hard_utility[0];   // (a NaN utility compares false)
  a.improved_hard[0] = improved ? 1 : 0;
  if (improved) {
    a.best_hard_utility[0] = util;
    a.best_hard_epoch[0] = e;
  }
}

// the jobs handed over with the launch (buffers whose address changes from
// step to step in an eager loop; fixed by the capture in a replayed one)
struct ExtraJobs {
  pfsgnn_copy_job j[PFSGNN_COPY_EXTRA_MAX];
};

// blockIdx.y: the job (the device list first, then the extra ones);
// blockIdx.x strides over its words
__global__ __launch_bounds__(256) void k_copy_if(const int* __restrict__ flag,
                                                 const pfsgnn_copy_job* __restrict__ jobs,
                                                 int njobs, ExtraJobs extra) {
  if (flag[0] == 0) return;
  pfsgnn_copy_job j;
  if ((int)blockIdx.y < njobs) {
    j = jobs[blockIdx.y];
  } else {
    const int x = (int)blockIdx.y - njobs;
    j = extra.j[0];
#pragma unroll
    for (int i = 1; i < PFSGNN_COPY_EXTRA_MAX; ++i)
      if (x == i) j = extra.j[i];
  }
  const long long stride = (long long)gridDim.x * 256;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const uint32_t* s = reinterpret_cast<const uint32_t*>(j.src);
  uint32_t* d = reinterpret_cast<uint32_t*>(j.dst);
  long long done = 0;
  if ((((uintptr_t)j.src | (uintptr_t)j.dst) & 15) == 0) {
    const long long n4 = j.n >> 2;
    const uint4* s4 = reinterpret_cast<const uint4*>(j.src);
    uint4* d4 = reinterpret_cast<uint4*>(j.dst);
    for (long long k = i; k < n4; k += stride) d4[k] = s4[k];
    done = n4 << 2;
  }
  for (long long k = done + i; k < j.n; k += stride) d[k] = s[k];
}

extern "C" int pfsgnn_softfloor_record(const float* sharpness, float* sf, void* stream) {
  PF_REQUIRE(sharpness && sf, "pfsgnn_softfloor_record", "null");
  PF_REQUIRE(((uintptr_t)sf & 15) == 0, "pfsgnn_softfloor_record", "sf must be 16-byte aligned");
  hipLaunchKernelGGL(k_softfloor_record, dim3(1), dim3(64), 0, as_stream(stream), sharpness,
                     reinterpret_cast<SoftFloor*>(sf));
  return pf::check_launch("pfsgnn_softfloor_record");
}

extern "C" int pfsgnn_train_advance(long long* epoch, unsigned long long* seed, double s0,
                                    double s1, long long nepochs, float* sharpness, float* sf,
                                    void* stream) {
  PF_REQUIRE(epoch && seed && sharpness && sf, "pfsgnn_train_advance", "null");
  PF_REQUIRE(nepochs > 0, "pfsgnn_train_advance", "nepochs must be positive");
  PF_REQUIRE(((uintptr_t)sf & 15) == 0, "pfsgnn_train_advance", "sf must be 16-byte aligned");
  hipLaunchKernelGGL(k_train_advance, dim3(1), dim3(64), 0, as_stream(stream), epoch, seed, s0, s1,
                     nepochs, sharpness, reinterpret_cast<SoftFloor*>(sf));
  return pf::check_launch("pfsgnn_train_advance");
}

extern "C" size_t pfsgnn_train_record_args_bytes(void) { return sizeof(pfsgnn_train_record_args); }

extern "C" int pfsgnn_train_record(const pfsgnn_train_record_args* a, void* stream) {
  PF_REQUIRE(a, "pfsgnn_train_record", "null argument struct");
  PF_REQUIRE(a->G > 0 && a->NC > 0 && a->nepochs > 0, "pfsgnn_train_record", "bad dims");
  PF_REQUIRE(a->epoch && a->sharpness && a->loss && a->utils && a->variance && a->n_prime &&
                 a->ci && a->losses && a->objective && a->variances && a->comp && a->improved &&
                 a->best_utility && a->best_loss && a->best_epoch,
             "pfsgnn_train_record", "null");
  hipLaunchKernelGGL(k_train_record, dim3(1), dim3(256), 0, as_stream(stream), *a);
  return pf::check_launch("pfsgnn_train_record");
}

extern "C" size_t pfsgnn_train_record_hard_args_bytes(void) {
  return sizeof(pfsgnn_train_record_hard_args);
}

extern "C" int pfsgnn_train_record_hard(const pfsgnn_train_record_hard_args* a, void* stream) {
  PF_REQUIRE(a, "pfsgnn_train_record_hard", "null argument struct");
  PF_REQUIRE(a->G > 0 && a->nepochs > 0, "pfsgnn_train_record_hard", "bad dims");
  PF_REQUIRE(a->epoch && a->utility && a->over && a->hard_objective && a->hard_overtime &&
                 a->improved_hard && a->best_hard_utility && a->best_hard_epoch,
             "pfsgnn_train_record_hard", "null");
  hipLaunchKernelGGL(k_train_record_hard, dim3(1), dim3(64), 0, as_stream(stream), *a);
  return pf::check_launch("pfsgnn_train_record_hard");
}

extern "C" int pfsgnn_copy_if(const int* flag, const pfsgnn_copy_job* jobs, int njobs,
                              const pfsgnn_copy_job* extra, int nextra, long long max_n,
                              void* stream) {
  PF_REQUIRE(flag, "pfsgnn_copy_if", "null");
  PF_REQUIRE(njobs >= 0 && njobs <= 65000 && (njobs == 0 || jobs), "pfsgnn_copy_if",
             "bad device job list");
  PF_REQUIRE(nextra >= 0 && nextra <= PFSGNN_COPY_EXTRA_MAX && (nextra == 0 || extra),
             "pfsgnn_copy_if", "bad extra job list (at most PFSGNN_COPY_EXTRA_MAX)");
  PF_REQUIRE(njobs + nextra > 0 && max_n >= 0, "pfsgnn_copy_if", "no jobs");
  ExtraJobs x = {};
  for (int i = 0; i < nextra; ++i) {
    PF_REQUIRE(extra[i].n >= 0 && extra[i].n <= max_n && (extra[i].n == 0 || (extra[i].src && extra[i].dst)),
               "pfsgnn_copy_if", "bad extra job");
    x.j[i] = extra[i];
  }
  long long nbx = (max_n / 4 + 255) / 256;   // one 16-byte word per thread and pass
  nbx = nbx < 1 ? 1 : (nbx > 256 ? 256 : nbx);
  hipLaunchKernelGGL(k_copy_if, dim3((unsigned)nbx, (unsigned)(njobs + nextra)), dim3(256), 0,
                     as_stream(stream), flag, jobs, njobs, x);
  return pf::check_launch("pfsgnn_copy_if");
}
