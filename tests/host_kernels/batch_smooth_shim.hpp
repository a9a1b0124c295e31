// What csrc/batch_smooth.hpp takes from batch_smc.hpp and the headers behind it, as host code: tests/test_batch_smooth_kernel_text_host.py
// compiles the kernels' own text against this file (its `#include "batch_smc.hpp"` line names this header instead) into a stand-alone
// program.  A workgroup is kThreads host threads: __syncthreads is a barrier over all of them, __shfl and wave_sum_u64 exchange through
// one slot a lane with a barrier over the wavefront's 64 threads, __shared__ arrays are statics (one workgroup runs at a time), blockIdx,
// gridDim and threadIdx are per-thread variables the launcher sets.  fix_weight, the Philox block and the 53-bit uniform are the
// oracle's (oracle/cpprob_oracle.c), so the reference and this program draw the same bits.
#pragma once
#include <pthread.h>
#include <unistd.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" {
void orc_draw_block(uint64_t seed, uint64_t group, uint64_t draw, uint32_t out[4]);
double orc_u01_53(uint32_t lo, uint32_t hi);
uint32_t orc_fix_weight(double lw, double ref);
}

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static

namespace hostk {
struct Dim3 { unsigned x = 0, y = 0, z = 0; };
constexpr int kGroupThreads = 256, kGroupWave = 64, kGroupWaves = kGroupThreads / kGroupWave;

// One workgroup's shared state.  A slot is written again two exchanges later: every lane of the wavefront has then passed the
// barrier of the exchange in between, that is, has read what it wanted of the earlier one.
struct Group {
    pthread_barrier_t all;
    pthread_barrier_t wave[kGroupWaves];
    uint64_t slot[2][kGroupThreads];
    double* dynamic_lds = nullptr;             // the launch's dynamic LDS: a heap block of exactly its size
    long skew_us = 0;                          // threads 0 .. 7 leave every __syncthreads this late (an adversarial schedule)
};
inline Group g_group;
inline thread_local unsigned t_parity = 0;

inline void group_init()
{
    pthread_barrier_init(&g_group.all, nullptr, kGroupThreads);
    for (pthread_barrier_t& w : g_group.wave) pthread_barrier_init(&w, nullptr, kGroupWave);
}
inline double* dynamic_lds() { return g_group.dynamic_lds; }
}  // namespace hostk

inline thread_local hostk::Dim3 blockIdx, gridDim, threadIdx;

inline void __syncthreads()
{
    pthread_barrier_wait(&hostk::g_group.all);
    // a barrier orders nothing after it: the threads that reduce the wavefronts' partial results fall behind the others
    if (hostk::g_group.skew_us > 0 && threadIdx.x < 8) usleep((useconds_t)hostk::g_group.skew_us);
}

namespace hostk {
inline uint64_t exchange(uint64_t mine, int src_lane)
{
    const unsigned w = threadIdx.x / kGroupWave, p = t_parity;
    t_parity ^= 1u;
    g_group.slot[p][threadIdx.x] = mine;
    pthread_barrier_wait(&g_group.wave[w]);
    return g_group.slot[p][w * kGroupWave + ((unsigned)src_lane & (kGroupWave - 1))];
}
}  // namespace hostk

template <class T> inline T __shfl(T v, int src_lane)
{
    static_assert(sizeof(T) <= 8, "one 64-bit slot a lane");
    uint64_t bits = 0;
    std::memcpy(&bits, &v, sizeof(T));
    bits = hostk::exchange(bits, src_lane);
    std::memcpy(&v, &bits, sizeof(T));
    return v;
}

namespace cph {
constexpr int kWave = hostk::kGroupWave;
constexpr int kThreads = hostk::kGroupThreads;
constexpr int kWaves = kThreads / kWave;
constexpr int kPPT = 4;
constexpr int kTile = kThreads * kPPT;
constexpr int kBatchTab = 8;

inline int lane_id() { return (int)(threadIdx.x & (kWave - 1)); }
inline int wave_id() { return (int)(threadIdx.x >> 6); }

struct u32x4 { uint32_t x, y, z, w; };
inline u32x4 draw_block(uint64_t seed, uint64_t group, uint64_t draw)
{
    uint32_t r[4];
    orc_draw_block(seed, group, draw, r);
    return u32x4{r[0], r[1], r[2], r[3]};
}
inline double u01_53(uint32_t lo, uint32_t hi) { return orc_u01_53(lo, hi); }
inline uint32_t fix_weight(double lw, double ref) { return orc_fix_weight(lw, ref); }
inline double u64_to_double(uint64_t c) { return (double)c; }       // (one rounding, as the device's fused form)
inline double dmul_rn(double a, double b) { return a * b; }         // (built with -ffp-contract=off)

// every lane's total of the wavefront's 64 values
inline uint64_t wave_sum_u64(uint64_t v)
{
    const unsigned w = threadIdx.x / kWave, p = hostk::t_parity;
    (void)hostk::exchange(v, 0);
    uint64_t tot = 0;
    for (int l = 0; l < kWave; ++l) tot += hostk::g_group.slot[p][w * kWave + l];
    return tot;
}

template <class T> inline void lane_fill(T (&v)[kPPT], T x)
{
    for (int k = 0; k < kPPT; ++k) v[k] = x;
}
}  // namespace cph
