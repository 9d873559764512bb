// msm_kernels.inc -- Pippenger multi-scalar multiplication on BN254 G1 / G2 for gfx950.
//
// Replaces ParallelMultiexp<Curve>::multiexp (rust-rapidsnark/rapidsnark/src/multiexp.cpp:183-245):
// processChunk's scatter of mixed adds into per-thread bucket arrays (:46-71), packThreads
// (:109-130), the recursive-halving bucket reduction (:133-180) and the Horner combine (:236-242).
//
// The result is the same group element; after affine normalisation it is bit-identical to the
// reference's for every input, because EC addition is associative/commutative and every
// exceptional case (P+P, P+(-P), infinity, (0,0) bases) goes through the same branches as
// curve.cpp:185-250.  The schedule is GPU-native instead of a translation:
//
//   K1  bucket sort            (point, window) pairs grouped by bucket key (w, d), d != 0: two-level counting
//                              sort with LDS histograms (k_part, k_part_bins); no per-element global atomics
//   K2  bucket accumulate      one lane per <= 32-entry segment of a bucket, longest segments first: mixed adds
//                              in registers on the radix-2^29 field (G1: Fq9, G2: Fq2n)
//   K2' segment fold           multi-segment buckets (skewed witness scalars) by size class: lane / workgroup /
//                              64 workgroups
//   K4  weighted bucket sum    sum_d d*B_d per window: one running-sum level + per-(window, bit) tree sums
//   --  Horner over windows    <= 220 XYZZ points, on the host (negligible)
//
// Signed c-bit digits (for_signed_digits), c chosen from n (the reference's rule caps at 16 as well).
#include <stdio.h>
#include <chrono>
#include <stdlib.h>
#include <string.h>
#include "ctx.h"
#include "bn254_fq2pair.h"
#include "bn254_fq9.h"

using namespace k16;

namespace {

constexpr unsigned MIN_SEG   = 32;  // points per accumulate segment: short chains keep skewed inputs parallel;
constexpr unsigned MAX_SEG   = 1024; // grows with n / 2^c so that a typical bucket stays one segment
constexpr unsigned FOLD_SMALL = 16; // buckets with <= this many segments are folded by one lane
constexpr unsigned WSUM_MLOG_MAX = 5; // up to 2^5 slots per lane (default cap 8, ctx->wsum_mlog_cap) in the first weighted-sum level (fewer when that
                                      // would leave the GPU with too few lanes: the stage is latency-bound)
constexpr unsigned MAX_C     = 16;
constexpr unsigned MIN_C     = 4;

// windows of c bits over 256-bit scalars, plus one for the final carry of the signed recoding
__host__ __device__ inline unsigned n_windows(unsigned c) { return (256 + c - 1) / c + 1; }

// Workgroup barrier that first drains this wave's LDS queue.  hipcc 7.2 (gfx950) was observed to drop the
// s_waitcnt lgkmcnt(0) of __syncthreads() after a loop whose last instruction is a no-return LDS atomic
// (ds_add_u32): other waves then read the histogram before the add has landed (1-5 % of launches lost a few
// counts in k_part_bins).  The explicit wait makes every barrier in this file independent of that.
__device__ __forceinline__ void k16_lds_sync()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
}

// Wave priority for every kernel of an MSM except the bucket accumulation.  VALU issue on a SIMD is arbitrated by priority,
// then age (MI355X_MICROARCH.md): beside three long-lived accumulate waves a younger wave of another lane's sort / fold /
// reduction only got the issue slots those left over -- kernel traces show a 12-register, 30-us kernel taking 500 us next
// to an accumulation.  These kernels are short and (the sort) mostly wait on memory, so letting them win the arbitration
// costs the accumulation little and shortens every lane's chain.  K16_NO_SETPRIO=1 at build time (-D) to compare.
__device__ __forceinline__ void k16_short_kernel_prio()
{
#ifndef K16_NO_SETPRIO
#ifndef K16_SHORT_PRIO
#define K16_SHORT_PRIO 3
#endif
    __builtin_amdgcn_s_setprio(K16_SHORT_PRIO);
#endif
}

// Wave priority of the G2 bucket accumulation (lane pairs): in a proof it is 5 % of the H MSM's work but a long chain of its own
// (B2: accumulation + fold + weighted sum end ~0.6 ms after the polynomial chain, and the H accumulation starts when they do,
// profiles/r06/proof_timeline_8queues_variant0.txt), walked beside NTT passes that run at priority 3.  -DK16_G2_ACC_PRIO=n to compare.
#ifndef K16_G2_ACC_PRIO
#define K16_G2_ACC_PRIO 0
#endif
#ifndef K16_G1_ACC_PRIO
#define K16_G1_ACC_PRIO 0
#endif
template <class E>
__device__ __forceinline__ void k16_acc_prio()
{
    if constexpr (E::ALPP == 2) {
        if (K16_G2_ACC_PRIO) __builtin_amdgcn_s_setprio(K16_G2_ACC_PRIO);
    } else {
        if (K16_G1_ACC_PRIO) __builtin_amdgcn_s_setprio(K16_G1_ACC_PRIO);
    }
}

// ------------------------------------------------------------------------------------------
// K1: digit extraction.  Scalars are 32 B little-endian standard form (multiexp.cpp:26-41 reads
// an unaligned u64 at bit w*c; the last window is narrower because bits >= 256 are zero).
// ------------------------------------------------------------------------------------------
template <unsigned C>
__device__ __forceinline__ uint32_t digit_of(const uint32_t (&k)[8], unsigned w)
{
    const unsigned bit = w * C;
    const unsigned wd  = bit >> 5;
    const unsigned sh  = bit & 31;
    uint64_t       v   = k[wd];
    if (wd + 1 < 8) v |= (uint64_t)k[wd + 1] << 32;
    return (uint32_t)(v >> sh) & ((1u << C) - 1u);
}

// Signed-digit recoding: v = raw window + carry; a value above 2^(c-1) stands for the negative digit v - 2^c (carry 1
// into the next window).  A digit of magnitude m in 1 .. 2^(c-1) goes to bucket m - 1 of its window whatever its sign;
// the sign travels with the sorted entry (bit 31) and the accumulation negates the point's y when it gathers the row.
// So a window has 2^(c-1) buckets, all of them weighted sums of POSITIVE multiples, and the reduction needs no pairing.
// f(w, m1, neg) is called with m1 = m - 1 for every non-zero digit, including the carry window w = W.
template <unsigned C, class Fn>
__device__ __forceinline__ void for_signed_digits(const uint32_t (&k)[8], Fn f)
{
    constexpr unsigned W    = (256 + C - 1) / C;
    constexpr uint32_t HALF = 1u << (C - 1), FULL = 1u << C;
    uint32_t           carry = 0;
#pragma unroll
    for (unsigned w = 0; w < W; w++) {
        const uint32_t v   = digit_of<C>(k, w) + carry;   // 0 .. 2^c
        const uint32_t neg = v > HALF ? 1u : 0u;
        carry              = neg;
        const uint32_t m   = neg ? FULL - v : v;          // 0 .. 2^(c-1)
        if (m) f(w, m - 1u, neg);
    }
    if (carry) f(W, 0u, 0u);
}

// Fixed-base ("flat") variant: W = ceil(257 / C) digit positions, no carry window -- the digit positions cover 257 bits,
// so the top one has at most C-1 significant bits and the recoding cannot carry out of it.
template <unsigned C, class Fn>
__device__ __forceinline__ void for_signed_digits_flat(const uint32_t (&k)[8], Fn f)
{
    constexpr unsigned W    = (257 + C - 1) / C;
    constexpr uint32_t HALF = 1u << (C - 1), FULL = 1u << C;
    uint32_t           carry = 0;
#pragma unroll
    for (unsigned w = 0; w < W; w++) {
        const uint32_t raw = w * C < 256 ? digit_of<C>(k, w) : 0u;
        const uint32_t v   = raw + carry;
        const uint32_t neg = v > HALF ? 1u : 0u;
        carry              = neg;
        const uint32_t m   = neg ? FULL - v : v;
        if (m) f(w, m - 1u, neg);
    }
}

template <unsigned C, bool SCATTER>
__global__ void __launch_bounds__(256) k_digits(const uint4* __restrict__ scalars, uint64_t n,
                                                uint32_t* __restrict__ counts_or_cursor,
                                                uint32_t* __restrict__ sorted, const uint32_t* __restrict__ remap)
{
    k16_short_kernel_prio();
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint4    lo = scalars[2 * i], hi = scalars[2 * i + 1];
        uint32_t k[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        for_signed_digits<C>(k, [&](unsigned w, uint32_t m1, uint32_t neg) {
            uint32_t key = (w << (C - 1)) + m1;
            if (SCATTER) {
                uint32_t pos = atomicAdd(&counts_or_cursor[key], 1u);
                sorted[pos]  = (neg << 31) | (remap ? remap[i] : (uint32_t)i);
            } else {
                atomicAdd(&counts_or_cursor[key], 1u);
            }
        });
    }
}

// 16-byte vector loads / stores of whole points
template <class T>
__device__ __forceinline__ T load_vec(const T* __restrict__ p)
{
    static_assert(sizeof(T) % 16 == 0, "16-byte granularity");
    T            r;
    const uint4* s = reinterpret_cast<const uint4*>(p);
    uint4*       d = reinterpret_cast<uint4*>(&r);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 16; i++) d[i] = s[i];
    return r;
}
template <class T>
__device__ __forceinline__ void store_vec(T* __restrict__ p, const T& v)
{
    static_assert(sizeof(T) % 16 == 0, "16-byte granularity");
    uint4*       d = reinterpret_cast<uint4*>(p);
    const uint4* s = reinterpret_cast<const uint4*>(&v);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 16; i++) d[i] = s[i];
}

// ------------------------------------------------------------------------------------------
// K1 (fast path, n <= 2^24): two-level counting sort without per-element global atomics.
// Device-scope atomics execute at the memory side on MI355X (~15 G random 4-byte atomics/s measured),
// which made the histogram + scatter passes above the largest item of the MSM.  Here:
//   pass 1/2  a workgroup histograms a tile of 2048 points x W windows into LDS bins
//             (window, high digit bits); one global atomic per NON-EMPTY BIN PER TILE reserves the
//             tile's slice of the bin, and the tile's entries (low digit byte << 24 | point index) are
//             ranked with LDS atomics and written there (runs of ~8 entries)
//   pass 3    one workgroup per bin: LDS histogram over the low digit byte gives counts[] and
//             offsets[] of the bin's <= 256 buckets directly (bucket keys are bin-major, so no global
//             scan over the 2^20 keys is needed), then the entries are ranked again in LDS and the
//             final point-index lists are written.
// Identical outputs (counts, offsets, index lists up to order inside a bucket) as the generic path.
// ------------------------------------------------------------------------------------------
#ifndef K16_PART_TILE
#define K16_PART_TILE 2048
#endif
constexpr unsigned PART_TILE = K16_PART_TILE; // (lab builds override it; the packed 16-bit tile histograms need TILE * W < 65536)

// Entry of the partition: sign << 31 | low bucket bits << SHIFT | payload (point index, or table row for a flat MSM)
template <unsigned CC>
struct PartCfg {
    static constexpr unsigned C   = CC;
    static constexpr unsigned W   = (256 + C - 1) / C + 1; // incl. the carry window
    static constexpr unsigned BB  = C - 1;                 // bucket bits per window (magnitude - 1)
    static constexpr unsigned LO  = BB > 7 ? 7 : BB;
    static constexpr unsigned LO4 = LO;
    static constexpr unsigned HI  = BB - LO;
    static constexpr unsigned NB1 = W << HI;
    static constexpr unsigned SHIFT = 24;                   // 24-bit point index, 7 low bucket bits, sign
    static constexpr bool     FLAT  = false;
    static constexpr unsigned TILE  = PART_TILE;
};
// Fixed-base MSM over precomputed window tables (row w*n + i = 2^(C*w) * P_i): ONE bucket set for all digit positions,
// so the bucket is the magnitude alone and the entry carries the table row (25 bits: n * W < 2^25), 6 low bucket bits.
template <unsigned CC>
struct PartCfgFlat {
    static constexpr unsigned C   = CC;
    static constexpr unsigned W   = (257 + C - 1) / C;
    static constexpr unsigned BB  = C - 1;
    static constexpr unsigned LO  = 6;
    static constexpr unsigned LO4 = LO;
    static constexpr unsigned HI  = BB - LO;
    static constexpr unsigned NB1 = 1u << HI;
    static constexpr unsigned SHIFT = 25;
    static constexpr bool     FLAT  = true;
    // (8192 bins at c = 20: a 2048-point tile puts only ~3 entries into a bin -- 8.4 M global reservations for the
    // 2^21-point H MSM.  A 4096-point tile halves them and doubles the run length; measured: 378 vs 397 us for the
    // scatter pass, no gain -- the pass is bound by its two workgroups per CU, not by the reservations.)
    static constexpr unsigned TILE  = PART_TILE;
};

// Exclusive scan of the <= 8192 bin counts of the partition into LDS, by one 256-thread workgroup (thread t owns `per`
// consecutive bins).  SLICES: scan ceil(count / PART_SLICE) instead (a bin of s entries is processed by that many
// workgroups in pass 3).  Returns the grand total through *total (LDS).
constexpr unsigned PART_SLICE = 8192;
template <bool SLICES>
__device__ __forceinline__ void part_scan_lds(const uint32_t* __restrict__ gcount, uint32_t nb1, uint32_t* __restrict__ out,
                                              uint32_t* __restrict__ sh /* [256] */, uint32_t* __restrict__ total)
{
    const unsigned per = (nb1 + 255) / 256;
    uint32_t       sum = 0;
    for (unsigned j = 0; j < per; j++) {
        unsigned b = threadIdx.x * per + j;
        uint32_t v = b < nb1 ? gcount[b] : 0u;
        sum += SLICES ? (v + PART_SLICE - 1) / PART_SLICE : v;
    }
    sh[threadIdx.x] = sum;
    k16_lds_sync();
    for (unsigned o = 1; o < 256; o <<= 1) {
        uint32_t t = threadIdx.x >= o ? sh[threadIdx.x - o] : 0u;
        k16_lds_sync();
        sh[threadIdx.x] += t;
        k16_lds_sync();
    }
    uint32_t run = sh[threadIdx.x] - sum;
    if (threadIdx.x == 255) *total = sh[255];
    for (unsigned j = 0; j < per; j++) {
        unsigned b = threadIdx.x * per + j;
        if (b < nb1) {
            out[b]     = run;
            uint32_t v = gcount[b];
            run += SLICES ? (v + PART_SLICE - 1) / PART_SLICE : v;
        }
    }
    k16_lds_sync();
}

// conv_in != nullptr (counting pass of a G1 MSM whose table comes in the reference's format): the tile's points are
// also converted to the packed R' rows the accumulation gathers (k_convert_bases' job) -- as a kernel of its own that
// conversion sat in front of every lane's chain and cost 4 % of the pipelined throughput.
//
// SCATTER pass: ONE tile per workgroup (gridDim.x = number of tiles).  Every workgroup first scans the bin counts of the
// counting pass into LDS itself (17 KB of L2 reads and ~40 LDS steps, instead of a single-workgroup kernel between the
// two passes that every lane's chain had to wait for); a tile's slice of bin b then starts at  start[b] + (what the
// tiles before it -- in atomic order -- took), the latter from a zero-based global cursor.  Workgroup 0 also writes the
// bin starts and the slice table pass 3 needs.
//
// HS (counting pass of the prover's H MSM): the scalars do not exist yet -- scalar i is fromMontgomery(a[i] * b[i] - c[i])
// (groth16.cpp:266-275) of the three coset evaluations (packed R' values of Fr), formed here, written to `scalars` for the
// later passes and counted in the same breath: the kernel that used to produce them wrote 64 MB for this pass to read back,
// one launch earlier on the proof's critical path (VERDICT r3 item 2b).
__device__ __forceinline__ k16::Fr hs_scalar(const k16::Fr* __restrict__ a, const k16::Fr* __restrict__ b,
                                             const k16::Fr* __restrict__ c, uint64_t i)
{
    auto ld9 = [](const k16::Fr* p) -> k16::Fr9 {
        const uint4* s4 = reinterpret_cast<const uint4*>(p);
        const uint4  x = s4[0], y = s4[1];
        const uint32_t w[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
        return k16::fr9_load(w);
    };
    return k16::fr9_to_standard(k16::frsub9(k16::frmul9(ld9(&a[i]), ld9(&b[i])), ld9(&c[i])));
}
__global__ void __launch_bounds__(256) k_hs_fill(uint4* __restrict__ scalars, uint64_t n, const k16::Fr* __restrict__ a,
                                                 const k16::Fr* __restrict__ b, const k16::Fr* __restrict__ c)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const k16::Fr v = hs_scalar(a, b, c, i);
    scalars[2 * i]     = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
    scalars[2 * i + 1] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
}

template <class P, bool SCATTER, bool CONV = false, bool HS = false>
__global__ void __launch_bounds__(256) k_part(const uint4* __restrict__ scalars, uint64_t n, uint32_t* __restrict__ g,
                                              uint32_t* __restrict__ part, const k16::Aff<k16::Fq>* __restrict__ conv_in,
                                              k16::Aff<k16::Fq>* __restrict__ conv_out, const uint32_t* __restrict__ gcount,
                                              uint32_t* __restrict__ gstart, uint32_t* __restrict__ gslice,
                                              const uint64_t* __restrict__ skip = nullptr,
                                              const k16::Fr* __restrict__ hs_a = nullptr, const k16::Fr* __restrict__ hs_b = nullptr,
                                              const k16::Fr* __restrict__ hs_c = nullptr)
{
    static_assert(!HS || (!SCATTER && !CONV), "the H scalars are formed by the plain counting pass");
    // skip: bit i set = point i is left out of the sort (its table row is (0,0): k16_msm_zero_row_mask) -- both passes
    k16_short_kernel_prio();
    extern __shared__ uint32_t  part_lds[];
    __shared__ uint32_t         sh[256];
    __shared__ uint32_t         s_total;
    // the tile's histogram is kept as packed 16-bit counters, two bins per LDS word (a tile has at most 2048 x 17 entries),
    // the bin offsets as 32-bit words: 6 bytes per bin instead of 8 -- at the 8192 bins of the fixed-base c = 20 partition
    // three workgroups fit a CU instead of two
    constexpr unsigned          HW = (P::NB1 + 1) / 2;
    uint32_t*                   hist = part_lds;
    uint32_t*                   base = part_lds + HW;
    auto hadd = [&](uint32_t b) -> uint32_t { // returns the bin's count before the increment
        const unsigned sh16 = (b & 1u) << 4;
        return (atomicAdd(&hist[b >> 1], 1u << sh16) >> sh16) & 0xffffu;
    };
    auto hget = [&](uint32_t b) -> uint32_t { return (hist[b >> 1] >> ((b & 1u) << 4)) & 0xffffu; };
    const uint32_t              ntiles = (uint32_t)((n + P::TILE - 1) / P::TILE);
    // bin of (digit position w, key d), and the entry's payload: the point index, or the table row for a flat MSM
    auto bin_of = [](unsigned w, uint32_t m1) -> uint32_t { return P::FLAT ? (m1 >> P::LO) : ((w << P::HI) + (m1 >> P::LO)); };
    auto digits = [](const uint32_t (&k)[8], auto f) {
        if constexpr (P::FLAT)
            for_signed_digits_flat<P::C>(k, f);
        else
            for_signed_digits<P::C>(k, f);
    };
    if (SCATTER) {
        if (blockIdx.x == 0) { // the tables of pass 3 (slices first: `base` is reused for the starts)
            part_scan_lds<true>(gcount, P::NB1, base, sh, &s_total);
            for (unsigned b = threadIdx.x; b < P::NB1; b += blockDim.x) gslice[b] = base[b];
            if (threadIdx.x == 0) gslice[P::NB1] = s_total;
            k16_lds_sync();
        }
        part_scan_lds<false>(gcount, P::NB1, base, sh, &s_total);
        if (blockIdx.x == 0) {
            for (unsigned b = threadIdx.x; b < P::NB1; b += blockDim.x) gstart[b] = base[b];
            if (threadIdx.x == 0) gstart[P::NB1] = s_total;
        }
    }
    if constexpr (SCATTER) {
        // One tile per workgroup.  The tile's scalars are loaded ONCE, all of them before the first is used (eight
        // independent 32-byte loads per lane in flight instead of one per loop trip), and serve both the histogram and the
        // ranking pass; the global reservations of a lane's bins are issued back to back and waited for once (they used to
        // be 17 dependent round trips to the memory-side atomic unit per lane).
        constexpr unsigned PPT = P::TILE / 256;            // points per lane
        constexpr unsigned BPT = (P::NB1 + 255) / 256;     // bins per lane
        const uint32_t     tile = blockIdx.x;
        uint4              sc[PPT][2];
#pragma unroll
        for (unsigned p = 0; p < PPT; p++) {
            const uint64_t i = (uint64_t)tile * P::TILE + p * 256 + threadIdx.x;
            if (i < n && !(skip && ((skip[i >> 6] >> (i & 63u)) & 1ull))) {
                sc[p][0] = scalars[2 * i];
                sc[p][1] = scalars[2 * i + 1];
            } else {
                sc[p][0] = sc[p][1] = make_uint4(0u, 0u, 0u, 0u); // a zero scalar has no digits
            }
        }
        for (unsigned b = threadIdx.x; b < HW; b += blockDim.x) hist[b] = 0;
        k16_lds_sync();
#pragma unroll
        for (unsigned p = 0; p < PPT; p++) {
            uint32_t k[8] = {sc[p][0].x, sc[p][0].y, sc[p][0].z, sc[p][0].w, sc[p][1].x, sc[p][1].y, sc[p][1].z, sc[p][1].w};
            digits(k, [&](unsigned w, uint32_t m1, uint32_t) { (void)hadd(bin_of(w, m1)); });
        }
        k16_lds_sync();
        uint32_t got[BPT];
#pragma unroll
        for (unsigned j = 0; j < BPT; j++) {
            const unsigned b = threadIdx.x + j * 256;
            uint32_t       h = b < P::NB1 ? hget(b) : 0u;
            got[j]           = h ? atomicAdd(&g[b], h) : 0u;
        }
#pragma unroll
        for (unsigned j = 0; j < BPT; j++) {
            const unsigned b = threadIdx.x + j * 256;
            if (b < P::NB1) base[b] += got[j]; // start of the bin + what earlier tiles reserved
        }
        k16_lds_sync();
        for (unsigned b = threadIdx.x; b < HW; b += blockDim.x) hist[b] = 0;
        k16_lds_sync();
#pragma unroll
        for (unsigned p = 0; p < PPT; p++) {
            const uint64_t i = (uint64_t)tile * P::TILE + p * 256 + threadIdx.x;
            uint32_t k[8] = {sc[p][0].x, sc[p][0].y, sc[p][0].z, sc[p][0].w, sc[p][1].x, sc[p][1].y, sc[p][1].z, sc[p][1].w};
            digits(k, [&](unsigned w, uint32_t m1, uint32_t neg) {
                uint32_t b   = bin_of(w, m1);
                uint32_t r   = hadd(b);
                uint32_t row = P::FLAT ? (uint32_t)(w * n + i) : (uint32_t)i;
                part[base[b] + r] = (neg << 31) | ((m1 & ((1u << P::LO) - 1u)) << P::SHIFT) | row;
            });
        }
        return;
    }
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (unsigned b = threadIdx.x; b < HW; b += blockDim.x) hist[b] = 0;
        k16_lds_sync();
        for (unsigned p = 0; p < P::TILE / 256; p++) {
            const uint64_t i = (uint64_t)tile * P::TILE + p * 256 + threadIdx.x;
            if (i >= n) break;
            uint4 lo, hi;
            if constexpr (HS) {
                const k16::Fr v = hs_scalar(hs_a, hs_b, hs_c, i);
                lo = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
                hi = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
                uint4* out = const_cast<uint4*>(scalars);
                out[2 * i]     = lo;
                out[2 * i + 1] = hi;
            } else {
                lo = scalars[2 * i];
                hi = scalars[2 * i + 1];
            }
            uint32_t k[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            if (!(skip && ((skip[i >> 6] >> (i & 63u)) & 1ull)))
                digits(k, [&](unsigned w, uint32_t m1, uint32_t) { (void)hadd(bin_of(w, m1)); });
            if constexpr (CONV) {
                k16::Aff<k16::Fq> a = load_vec(&conv_in[i]);
                k16::Aff9         c9 = k16::aff9_from_canonical(a);
                k16::Aff<k16::Fq> o;
                k16::fq9_pack(o.x.v, c9.x);
                k16::fq9_pack(o.y.v, c9.y);
                store_vec(&conv_out[i], o);
            }
        }
        k16_lds_sync();
        for (unsigned b = threadIdx.x; b < P::NB1; b += blockDim.x) {
            uint32_t h = hget(b);
            if (h) atomicAdd(&g[b], h);
        }
        k16_lds_sync();
    }
}

constexpr unsigned WC_THREADS = 1024;
// exclusive starts of the partition's bins (and of their slices for pass 3): one workgroup, between the counting pass and
// the staged scatter pass (k_part_stage)
__global__ void __launch_bounds__(WC_THREADS) k_bin_starts(const uint32_t* __restrict__ gcount, uint32_t nb1,
                                                          uint32_t* __restrict__ gstart, uint32_t* __restrict__ gslice)
{
    k16_short_kernel_prio();
    __shared__ uint32_t sa[WC_THREADS], sb[WC_THREADS];
    const unsigned per = (nb1 + WC_THREADS - 1) / WC_THREADS;
    uint32_t       a = 0, b = 0;
    for (unsigned j = 0; j < per; j++) {
        const unsigned i = threadIdx.x * per + j;
        const uint32_t v = i < nb1 ? gcount[i] : 0u;
        a += v;
        b += (v + PART_SLICE - 1) / PART_SLICE;
    }
    sa[threadIdx.x] = a;
    sb[threadIdx.x] = b;
    k16_lds_sync();
    for (unsigned o = 1; o < WC_THREADS; o <<= 1) {
        const uint32_t ta = threadIdx.x >= o ? sa[threadIdx.x - o] : 0u, tb = threadIdx.x >= o ? sb[threadIdx.x - o] : 0u;
        k16_lds_sync();
        sa[threadIdx.x] += ta;
        sb[threadIdx.x] += tb;
        k16_lds_sync();
    }
    uint32_t ra = sa[threadIdx.x] - a, rb = sb[threadIdx.x] - b;
    for (unsigned j = 0; j < per; j++) {
        const unsigned i = threadIdx.x * per + j;
        if (i < nb1) {
            gstart[i]        = ra;
            gslice[i]        = rb;
            const uint32_t v = gcount[i];
            ra += v;
            rb += (v + PART_SLICE - 1) / PART_SLICE;
        }
    }
    if (threadIdx.x == WC_THREADS - 1) {
        gstart[nb1] = sa[WC_THREADS - 1];
        gslice[nb1] = sb[WC_THREADS - 1];
    }
}

// ------------------------------------------------------------------------------------------
// Staged scatter pass with FIVE-byte entries (round 4).  What the measurements of rounds 3-4 say about this pass: the
// memory side merges 4-byte stores only when they arrive close together -- the bucket pass, whose workgroups each fill a
// 13 KB region within microseconds, writes 1.04x its bytes, the scatter pass of k_part, whose (tile, bin) runs of 3-32
// entries are completed by other tiles much later, 6-9x (398-472 MB for 67 MB at 2^20 x c16, 1.0-1.15 GB for 109 MB in the H
// sort), and neither longer runs (PART_TILE 2048 ... 8192) nor per-XCD sub-regions of every bin (lines assembled in
// ONE L2) change that.  So a workgroup has to write whole sectors itself: the tile's entries are ranked into LDS in
// bin-major order and copied out by half-waves, one run at a time, adjacent lanes to adjacent addresses.  That only pays
// when a run is long, i.e. with FEW bins -- and a 32-bit entry (sign + low key bits + 25-bit row) forces 2^13 of them for
// the fixed-base H sort (45 bits of information, DESIGN 8.1).  Hence the fifth byte: a side array carries three more low
// key bits, the partition has 1024 bins, a 2048-point tile leaves runs of 26 entries (104 + 26 bytes), one global
// reservation per bin per tile instead of eight, and pass 3 ranks 512 buckets per bin (k_part_bins with `side`).
template <unsigned CC>
struct PartCfgFlat5 {
    static constexpr unsigned C   = CC;
    static constexpr unsigned W   = (257 + C - 1) / C;
    static constexpr unsigned BB  = C - 1;
    static constexpr unsigned LO  = 9;                      // 6 bits in the entry, 3 in the side byte
    static constexpr unsigned LO4 = 6;
    static constexpr unsigned HI  = BB - LO;
    static constexpr unsigned NB1 = 1u << HI;
    static constexpr unsigned SHIFT = 25;
    static constexpr bool     FLAT  = true;
    static constexpr unsigned TILE  = PART_TILE;            // the counting pass (k_part<P, false>)
#ifndef K16_ST_TILE_FLAT
#define K16_ST_TILE_FLAT 2048
#endif
    static constexpr unsigned ST_TILE = K16_ST_TILE_FLAT;   // points per workgroup of k_part_stage (2048: 145 KB of LDS)
};
// ordinary MSM at c = 16: 17 windows x 64 high-bit bins = 1088 bins (4352 with 4-byte entries), runs of 32 entries
template <unsigned CC>
struct PartCfg5 {
    static constexpr unsigned C   = CC;
    static constexpr unsigned W   = (256 + C - 1) / C + 1;
    static constexpr unsigned BB  = C - 1;
    static constexpr unsigned LO  = BB > 9 ? 9 : BB;         // 7 bits in the entry, 2 in the side byte
    static constexpr unsigned LO4 = 7;
    static constexpr unsigned HI  = BB - LO;
    static constexpr unsigned NB1 = W << HI;
    static constexpr unsigned SHIFT = 24;
    static constexpr bool     FLAT  = false;
    static constexpr unsigned TILE  = PART_TILE;
    static constexpr unsigned ST_TILE = 1024;               // (2048 points x 17 windows x 5 bytes do not fit the LDS)
};
constexpr unsigned ST_THREADS = 1024;
template <class P>
struct StageGeom {
    static constexpr unsigned CAP       = P::ST_TILE * P::W;                       // entries of a tile, at most
    static constexpr unsigned NBP       = (P::NB1 + ST_THREADS - 1) / ST_THREADS;  // bins per lane
    // LDS: cur[NB1] | toff[NB1 + 1] | gdl[NB1] | scan scratch[1024] | stage4[CAP] | stage1[CAP bytes]
    static constexpr unsigned LDS_BYTES = (3 * P::NB1 + 1 + ST_THREADS + CAP) * 4 + ((CAP + 3) & ~3u);
};
template <class P>
__global__ void __launch_bounds__(ST_THREADS) k_part_stage(const uint4* __restrict__ scalars, uint64_t n, uint32_t* __restrict__ g,
                                                           uint32_t* __restrict__ part4, uint8_t* __restrict__ part1,
                                                           const uint32_t* __restrict__ gstart)
{
    k16_short_kernel_prio();
    typedef StageGeom<P>       G;
    extern __shared__ uint32_t st_lds[];
    uint32_t* cur  = st_lds;                 // histogram, then the running rank of every bin
    uint32_t* toff = cur + P::NB1;           // [NB1 + 1] exclusive starts inside the tile
    uint32_t* gdl  = toff + P::NB1 + 1;      // where the tile's run of a bin starts in part4 / part1
    uint32_t* sh   = gdl + P::NB1;           // [1024]
    uint32_t* st4  = sh + ST_THREADS;        // [CAP]
    uint8_t*  st1  = reinterpret_cast<uint8_t*>(st4 + G::CAP);
    constexpr unsigned PPT = P::ST_TILE / ST_THREADS;
    auto bin_of = [](unsigned w, uint32_t m1) -> uint32_t { return P::FLAT ? (m1 >> P::LO) : ((w << P::HI) + (m1 >> P::LO)); };
    auto digits = [](const uint32_t (&k)[8], auto f) {
        if constexpr (P::FLAT)
            for_signed_digits_flat<P::C>(k, f);
        else
            for_signed_digits<P::C>(k, f);
    };
    const uint32_t tile = blockIdx.x;
    uint4          sc[PPT][2];
#pragma unroll
    for (unsigned p = 0; p < PPT; p++) {
        const uint64_t i = (uint64_t)tile * P::ST_TILE + p * ST_THREADS + threadIdx.x;
        if (i < n) {
            sc[p][0] = scalars[2 * i];
            sc[p][1] = scalars[2 * i + 1];
        } else {
            sc[p][0] = sc[p][1] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    for (unsigned b = threadIdx.x; b < P::NB1; b += ST_THREADS) cur[b] = 0;
    k16_lds_sync();
#pragma unroll
    for (unsigned p = 0; p < PPT; p++) {
        uint32_t k[8] = {sc[p][0].x, sc[p][0].y, sc[p][0].z, sc[p][0].w, sc[p][1].x, sc[p][1].y, sc[p][1].z, sc[p][1].w};
        digits(k, [&](unsigned w, uint32_t m1, uint32_t) { atomicAdd(&cur[bin_of(w, m1)], 1u); });
    }
    k16_lds_sync();
    // exclusive scan of the bin counts (lane t owns NBP consecutive bins), one reservation per non-empty bin
    {
        uint32_t h[G::NBP], sum = 0;
#pragma unroll
        for (unsigned j = 0; j < G::NBP; j++) {
            const unsigned b = threadIdx.x * G::NBP + j;
            h[j]             = b < P::NB1 ? cur[b] : 0u;
            sum += h[j];
        }
        sh[threadIdx.x] = sum;
        k16_lds_sync();
        for (unsigned o = 1; o < ST_THREADS; o <<= 1) {
            const uint32_t t = threadIdx.x >= o ? sh[threadIdx.x - o] : 0u;
            k16_lds_sync();
            sh[threadIdx.x] += t;
            k16_lds_sync();
        }
        uint32_t run = sh[threadIdx.x] - sum;
        uint32_t got[G::NBP];
#pragma unroll
        for (unsigned j = 0; j < G::NBP; j++) {
            const unsigned b = threadIdx.x * G::NBP + j;
            got[j]           = (b < P::NB1 && h[j]) ? atomicAdd(&g[b], h[j]) : 0u;
        }
#pragma unroll
        for (unsigned j = 0; j < G::NBP; j++) {
            const unsigned b = threadIdx.x * G::NBP + j;
            if (b < P::NB1) {
                cur[b]  = run;
                toff[b] = run;
                gdl[b]  = gstart[b] + got[j];
                run += h[j];
            }
        }
        if (threadIdx.x == ST_THREADS - 1) toff[P::NB1] = sh[ST_THREADS - 1];
    }
    k16_lds_sync();
#pragma unroll
    for (unsigned p = 0; p < PPT; p++) {
        const uint64_t i = (uint64_t)tile * P::ST_TILE + p * ST_THREADS + threadIdx.x;
        uint32_t k[8] = {sc[p][0].x, sc[p][0].y, sc[p][0].z, sc[p][0].w, sc[p][1].x, sc[p][1].y, sc[p][1].z, sc[p][1].w};
        digits(k, [&](unsigned w, uint32_t m1, uint32_t neg) {
            const uint32_t pos = atomicAdd(&cur[bin_of(w, m1)], 1u);
            const uint32_t row = P::FLAT ? (uint32_t)(w * n + i) : (uint32_t)i;
            const uint32_t lo  = m1 & ((1u << P::LO) - 1u);
            st4[pos] = (neg << 31) | ((lo & ((1u << P::LO4) - 1u)) << P::SHIFT) | row;
            st1[pos] = (uint8_t)(lo >> P::LO4);
        });
    }
    k16_lds_sync();
    // copy-out, one run per half-wave at a time: lanes 0 .. 31 store consecutive entries of the run
    const unsigned hw = threadIdx.x >> 5, l32 = threadIdx.x & 31u;
    for (unsigned b = hw; b < P::NB1; b += ST_THREADS / 32) {
        const uint32_t lo = toff[b], len = toff[b + 1] - lo, dst = gdl[b];
        for (uint32_t k = l32; k < len; k += 32) {
            part4[dst + k] = st4[lo + k];
            part1[dst + k] = st1[lo + k];
        }
    }
}

// pass 3, one workgroup per (bin, slice of <= PART_SLICE entries).
//   MODE 0 (count)    LDS histogram over the low digit bits -> global bucket counts
//   MODE 1 (scatter)  reserve each bucket's run with one global atomic per non-empty bucket per slice, rank the entries
//                     in LDS, write the final point-index lists
// Lanes that share the first active lane's key are ranked by ballot (skewed inputs put most of a bin into one bucket).
template <class P, int MODE>
__global__ void __launch_bounds__(256) k_part_bins(const uint32_t* __restrict__ gstart, const uint32_t* __restrict__ gslice,
                                                   uint32_t nb1, const uint32_t* __restrict__ part,
                                                   uint32_t* __restrict__ counts_or_cursor, uint32_t* __restrict__ sorted,
                                                   const uint32_t* __restrict__ remap,
                                                   const uint8_t* __restrict__ side = nullptr, uint32_t small_cap = 0,
                                                   const uint64_t* __restrict__ drop = nullptr)
{
    // drop: entries whose point has its bit set are left out -- a second set of bucket lists from another MSM's partition
    // for a table in which those rows are (0,0) (msm_sort_derive_launch)
    k16_short_kernel_prio();
    constexpr unsigned  LON = 1u << P::LO;
    constexpr unsigned  HN  = LON > 256 ? LON : 256;   // five-byte entries (PartCfg*5): 512 low keys, the upper bits in `side`
    constexpr bool      SIDE = LON > 128;
    constexpr unsigned  LO4  = P::LO4; // key bits inside the 32-bit entry
    __shared__ uint32_t h[HN], base[HN];
    __shared__ uint32_t s_bin;
    const uint32_t      g = blockIdx.x;
    if (g >= gslice[nb1]) return;
    if (threadIdx.x == 0) {
        uint32_t lo = 0, hi = nb1; // gslice[lo] <= g < gslice[hi]
        if (g < nb1 && gslice[g] == g && gslice[g + 1] > g) { // every bin before this one has exactly one slice
            lo = g;
        } else {
            while (hi - lo > 1) {
                uint32_t mid = (lo + hi) >> 1;
                if (gslice[mid] <= g) lo = mid; else hi = mid;
            }
        }
        s_bin = lo;
    }
    for (unsigned t = threadIdx.x; t < HN; t += 256) h[t] = 0;
    k16_lds_sync();
    const uint32_t bin    = s_bin;
    if (small_cap && gstart[bin + 1] - gstart[bin] <= small_cap) return; // finished by k_bins_stage
    const uint32_t s0  = gstart[bin] + (g - gslice[bin]) * PART_SLICE;
    const uint32_t s1  = min(s0 + PART_SLICE, gstart[bin + 1]);
    // the slice's entries (<= 32 per lane) are loaded once, all loads in flight together, and serve both passes: the
    // two loops used to pay one dependent global-load latency per 256 entries each (16 + 16 round trips for a 4096-entry bin)
    constexpr unsigned EPT = PART_SLICE / 256;
    uint32_t           ent[EPT];
    uint32_t           sdp[SIDE ? EPT / 4 : 1]; // side bytes, four to a register
    uint32_t           dropped = 0;             // bit k: entry k of this lane is left out
    static_assert(EPT <= 32, "one bit per entry of a lane");
#pragma unroll
    for (unsigned k = 0; k < EPT; k++) {
        const uint32_t j = s0 + k * 256 + threadIdx.x;
        ent[k]           = j < s1 ? part[j] : 0xffffffffu;
    }
    if (drop) {
#pragma unroll
        for (unsigned k = 0; k < EPT; k++) {
            const uint32_t j  = s0 + k * 256 + threadIdx.x;
            const uint32_t pt = ent[k] & ((1u << P::SHIFT) - 1u);
            if (j < s1 && ((drop[pt >> 6] >> (pt & 63u)) & 1ull)) dropped |= 1u << k;
        }
    }
    if constexpr (SIDE) {
#pragma unroll
        for (unsigned k = 0; k < EPT / 4; k++) sdp[k] = 0;
#pragma unroll
        for (unsigned k = 0; k < EPT; k++) {
            const uint32_t j = s0 + k * 256 + threadIdx.x;
            if (j < s1) sdp[k >> 2] |= (uint32_t)side[j] << ((k & 3u) * 8);
        }
    }
    auto low_key = [&](unsigned k, uint32_t e) -> uint32_t {
        if constexpr (SIDE)
            return ((e >> P::SHIFT) & ((1u << LO4) - 1u)) | (((sdp[k >> 2] >> ((k & 3u) * 8)) & 0xffu) << LO4);
        else
            return (e >> P::SHIFT) & (LON - 1u);
    };
#pragma clang loop unroll_count(EPT)
    for (unsigned k = 0; k < EPT; k++) {
        if (s0 + k * 256 >= s1) break; // workgroup-uniform
        const uint32_t j      = s0 + k * 256 + threadIdx.x;
        const bool     active = j < s1 && !((dropped >> k) & 1u);
        const uint32_t key    = active ? low_key(k, ent[k]) : 0xffffffffu;
        const uint32_t k0     = __builtin_amdgcn_readfirstlane(key);
        const uint64_t same   = __ballot(active && key == k0);
        if (active) {
            if (key == k0) {
                if ((uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0u)) == 0)
                    atomicAdd(&h[key], (uint32_t)__popcll(same));
            } else {
                atomicAdd(&h[key], 1u);
            }
        }
    }
    k16_lds_sync();
    if (MODE == 0) {
        for (unsigned t = threadIdx.x; t < LON; t += 256) {
            const uint32_t v = h[t];
            if (v) atomicAdd(&counts_or_cursor[bin * LON + t], v);
        }
        return;
    }
    for (unsigned t = threadIdx.x; t < HN; t += 256) {
        const uint32_t v = h[t];
        base[t] = (t < LON && v) ? atomicAdd(&counts_or_cursor[bin * LON + t], v) : 0u;
        h[t]    = 0;
    }
    k16_lds_sync();
#pragma clang loop unroll_count(EPT)
    for (unsigned k = 0; k < EPT; k++) {
        if (s0 + k * 256 >= s1) break;
        const uint32_t j      = s0 + k * 256 + threadIdx.x;
        const bool     active = j < s1 && !((dropped >> k) & 1u);
        const uint32_t e      = ent[k];
        const uint32_t key    = active ? low_key(k, e) : 0xffffffffu;
        const uint32_t k0     = __builtin_amdgcn_readfirstlane(key);
        const uint64_t same   = __ballot(active && key == k0);
        const uint32_t rank   = (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0u));
        uint32_t       pos    = 0;
        if (active && key != k0) pos = atomicAdd(&h[key], 1u);
        uint32_t grp = 0;
        if (active && key == k0 && rank == 0) grp = atomicAdd(&h[key], (uint32_t)__popcll(same));
        grp = __shfl(grp, same ? (int)__builtin_ctzll(same) : 0);
        if (active) {
            if (key == k0) pos = grp + rank;
            uint32_t out = e & (0x80000000u | ((1u << P::SHIFT) - 1u)); // sign + payload
            // the scalars are a compacted subset of the table's rows (the wide scalars of a witness): point k is row remap[k]
            if (remap) out = (out & 0x80000000u) | remap[out & 0x7fffffffu];
            sorted[base[key] + pos] = out;
        }
    }
}

// Pass 3 for the five-byte partition, one workgroup per BIN (round 4).  A bin of the 1024-bin partitions holds ~27 k
// entries for 512 buckets: as 8192-entry slices handled by unrelated workgroups its buckets would be written in runs of 16
// entries at different times -- the scatter pass's write amplification moved here (measured: 490 MB for 109 MB, 205 us).
// Here the workgroup that owns the bin ranks ALL of its entries into LDS in bucket order and copies the bin's stretch of
// the sorted array out as one contiguous, coalesced block; bucket counts are its LDS histogram, bucket offsets
// gstart[bin] + local prefix -- no global atomics, and the same values the global scan derives from the counts.  Bins with
// more than BS_CAP entries (the 32 bins the top window's short digits fall into, skewed inputs) are left to the sliced
// k_part_bins launches, which skip the others (small_cap).
constexpr unsigned BS_THREADS = 1024;
constexpr unsigned BS_CAP     = 32768;
template <class P>
__global__ void __launch_bounds__(BS_THREADS) k_bins_stage(const uint32_t* __restrict__ gstart, uint32_t nb1,
                                                           const uint32_t* __restrict__ part, const uint8_t* __restrict__ side,
                                                           uint32_t* __restrict__ counts, uint32_t* __restrict__ sorted,
                                                           const uint32_t* __restrict__ remap)
{
    k16_short_kernel_prio();
    constexpr unsigned LON = 1u << P::LO;
    static_assert(LON <= BS_THREADS, "one lane per bucket of the bin");
    extern __shared__ uint32_t bs_lds[];
    uint32_t* h     = bs_lds;            // [LON] histogram -> running rank
    uint32_t* sh    = h + LON;           // [BS_THREADS]
    uint32_t* stage = sh + BS_THREADS;   // [BS_CAP]
    const uint32_t bin = blockIdx.x;
    const uint32_t s0 = gstart[bin], s1 = gstart[bin + 1], E = s1 - s0;
    if (E == 0 || E > BS_CAP) return;
    constexpr unsigned EPT = BS_CAP / BS_THREADS;
    uint32_t           ent[EPT], sdp[EPT / 4];
#pragma unroll
    for (unsigned k = 0; k < EPT / 4; k++) sdp[k] = 0;
#pragma unroll
    for (unsigned k = 0; k < EPT; k++) {
        const uint32_t j = s0 + k * BS_THREADS + threadIdx.x;
        ent[k]           = j < s1 ? part[j] : 0u;
        if (j < s1) sdp[k >> 2] |= (uint32_t)side[j] << ((k & 3u) * 8);
    }
    auto low_key = [&](unsigned k) -> uint32_t {
        return ((ent[k] >> P::SHIFT) & ((1u << P::LO4) - 1u)) | (((sdp[k >> 2] >> ((k & 3u) * 8)) & 0xffu) << P::LO4);
    };
    for (unsigned t = threadIdx.x; t < LON; t += BS_THREADS) h[t] = 0;
    k16_lds_sync();
#pragma unroll
    for (unsigned k = 0; k < EPT; k++) {
        if (s0 + k * BS_THREADS >= s1) break; // workgroup-uniform
        if (s0 + k * BS_THREADS + threadIdx.x < s1) atomicAdd(&h[low_key(k)], 1u);
    }
    k16_lds_sync();
    {
        const uint32_t v = threadIdx.x < LON ? h[threadIdx.x] : 0u;
        if (threadIdx.x < LON) counts[bin * LON + threadIdx.x] = v;
        sh[threadIdx.x] = v;
        k16_lds_sync();
        for (unsigned o = 1; o < LON; o <<= 1) {
            const uint32_t t = (threadIdx.x >= o && threadIdx.x < LON) ? sh[threadIdx.x - o] : 0u;
            k16_lds_sync();
            if (threadIdx.x < LON) sh[threadIdx.x] += t;
            k16_lds_sync();
        }
        if (threadIdx.x < LON) h[threadIdx.x] = sh[threadIdx.x] - v; // exclusive start of the bucket inside the bin
    }
    k16_lds_sync();
#pragma unroll
    for (unsigned k = 0; k < EPT; k++) {
        if (s0 + k * BS_THREADS >= s1) break;
        if (s0 + k * BS_THREADS + threadIdx.x < s1) {
            const uint32_t pos = atomicAdd(&h[low_key(k)], 1u);
            uint32_t       out = ent[k] & (0x80000000u | ((1u << P::SHIFT) - 1u)); // sign + payload
            if (remap) out = (out & 0x80000000u) | remap[out & 0x7fffffffu];
            stage[pos] = out;
        }
    }
    k16_lds_sync();
    for (uint32_t j = threadIdx.x; j < E; j += BS_THREADS) sorted[s0 + j] = stage[j];
}

// ------------------------------------------------------------------------------------------
// Bucket offsets AND segment offsets in two launches: exclusive scans of counts[] and of ceil(counts[] / seg).
//   k_scan2_totals  per-block totals of both sequences
//   k_scan2_apply   every block sums the totals of the blocks before it (<= 4096 of them), rescans its own 4096
//                   elements and writes offsets[] (+ a copy that the final scatter advances), seg_off[], the two grand
//                   totals, and -- since it holds every bucket's segment count -- the size classes of the fold
// (Was: two three-kernel scans and a classification kernel; every launch in a lane's chain waits for a CU slot while
// another lane's accumulation owns the chip.)
// ------------------------------------------------------------------------------------------
constexpr unsigned SCAN_T   = 256;
// elements per thread of the two scan kernels (template parameter PER).  16 (4096-element blocks: 128 workgroups at 2^19
// buckets, four 64-byte-strided loads per lane and 16-deep serial loops) took 58 us of a 395-us sort; 4 (544 workgroups,
// one 16-byte load per lane) is what the launches use now.
constexpr unsigned SCAN_PER_DEFAULT = 4;

// Folding the segment partials of multi-segment buckets, by size class:
//   2 .. FOLD_SERIAL segments  one lane per bucket, serial adds
//   .. FOLD_SMALL (16)         16 lanes per bucket, 4-step shuffle tree      (from a list)
//   .. FOLD_GIANT              one workgroup per bucket, strided + LDS tree  (from a list)
//   more                       GIANT_BLOCKS workgroups per bucket + a second tiny pass (skewed witness
//                              scalars put ~45 % of all points into ONE bucket: 19 k partials at n = 1.3 M)
constexpr unsigned FOLD_SERIAL  = 4;    // <= this many segments: one lane adds them serially
constexpr unsigned FOLD_GIANT   = 2048;
constexpr unsigned GIANT_BLOCKS = 64;
constexpr unsigned GIANT_CAP    = 256;

// appends `value` of the lanes with pred to list[] (count is bumped by the whole group even when it does not fit);
// returns whether THIS lane's value was stored
__device__ __forceinline__ bool wave_append(bool pred, uint32_t value, uint32_t* __restrict__ list,
                                            uint32_t* __restrict__ count, uint32_t cap)
{
    const uint64_t m = __ballot(pred);
    if (!m) return false;
    const uint32_t rank = (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    uint32_t       base = 0;
    if (pred && rank == 0) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = __shfl(base, (int)__builtin_ctzll(m));
    const bool stored = pred && base + rank < cap;
    if (stored) list[base + rank] = value;
    return stored;
}

template <unsigned SCAN_PER>
__global__ void __launch_bounds__(SCAN_T) k_scan2_totals(const uint32_t* __restrict__ in, uint32_t n, uint32_t seg,
                                                         uint32_t* __restrict__ block_tot)
{
    k16_short_kernel_prio();
    constexpr unsigned  SCAN_BLK = SCAN_T * SCAN_PER;
    __shared__ uint32_t sa[SCAN_T], sb[SCAN_T];
    const uint32_t      base = blockIdx.x * SCAN_BLK + threadIdx.x * SCAN_PER;
    uint32_t            a = 0, b = 0;
#pragma unroll
    for (unsigned j = 0; j < SCAN_PER; j++) {
        uint32_t x = (base + j < n) ? in[base + j] : 0u;
        a += x;
        b += (x + seg - 1) / seg;
    }
    sa[threadIdx.x] = a;
    sb[threadIdx.x] = b;
    k16_lds_sync();
    for (unsigned o = SCAN_T >> 1; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            sa[threadIdx.x] += sa[threadIdx.x + o];
            sb[threadIdx.x] += sb[threadIdx.x + o];
        }
        k16_lds_sync();
    }
    if (threadIdx.x == 0) {
        block_tot[blockIdx.x]             = sa[0];
        block_tot[gridDim.x + blockIdx.x] = sb[0];
    }
}

// misc: [0] total entries, [1] total segments, [2] medium count, [3] giant count, [4] tree count
template <unsigned SCAN_PER>
__global__ void __launch_bounds__(SCAN_T) k_scan2_apply(const uint32_t* __restrict__ in, uint32_t n, uint32_t seg,
                                                        const uint32_t* __restrict__ block_tot, uint32_t* __restrict__ offsets,
                                                        uint32_t* __restrict__ cursor, uint32_t* __restrict__ seg_off,
                                                        uint32_t* __restrict__ misc, uint32_t* __restrict__ med_list,
                                                        uint32_t med_cap, uint32_t* __restrict__ giant_list,
                                                        uint32_t* __restrict__ tree_list, uint32_t* __restrict__ seg_bucket,
                                                        uint32_t* __restrict__ seg_hist)
{
    k16_short_kernel_prio();
    constexpr unsigned  SCAN_BLK = SCAN_T * SCAN_PER;
    __shared__ uint32_t sa[SCAN_T], sb[SCAN_T];
    __shared__ uint32_t lh[MAX_SEG + 1]; // segment-length histogram of this block's buckets
    for (unsigned i = threadIdx.x; i <= seg; i += SCAN_T) lh[i] = 0;
    // (1) totals of the blocks before this one
    uint32_t pa = 0, pb = 0;
    for (uint32_t j = threadIdx.x; j < blockIdx.x; j += SCAN_T) {
        pa += block_tot[j];
        pb += block_tot[gridDim.x + j];
    }
    sa[threadIdx.x] = pa;
    sb[threadIdx.x] = pb;
    k16_lds_sync();
    for (unsigned o = SCAN_T >> 1; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            sa[threadIdx.x] += sa[threadIdx.x + o];
            sb[threadIdx.x] += sb[threadIdx.x + o];
        }
        k16_lds_sync();
    }
    const uint32_t pre_a = sa[0], pre_b = sb[0];
    k16_lds_sync();
    // (2) this block's 4096 elements
    const uint32_t base = blockIdx.x * SCAN_BLK + threadIdx.x * SCAN_PER;
    uint32_t       va[SCAN_PER], vb[SCAN_PER], ns[SCAN_PER], xs[SCAN_PER];
    uint32_t       a = 0, b = 0;
#pragma unroll
    for (unsigned j = 0; j < SCAN_PER; j++) {
        uint32_t x = (base + j < n) ? in[base + j] : 0u;
        xs[j]      = x;
        ns[j]      = (x + seg - 1) / seg;
        va[j]      = a;
        vb[j]      = b;
        a += x;
        b += ns[j];
    }
    sa[threadIdx.x] = a;
    sb[threadIdx.x] = b;
    k16_lds_sync();
    for (unsigned o = 1; o < SCAN_T; o <<= 1) {
        uint32_t ta = (threadIdx.x >= o) ? sa[threadIdx.x - o] : 0u;
        uint32_t tb = (threadIdx.x >= o) ? sb[threadIdx.x - o] : 0u;
        k16_lds_sync();
        sa[threadIdx.x] += ta;
        sb[threadIdx.x] += tb;
        k16_lds_sync();
    }
    const uint32_t ea = pre_a + sa[threadIdx.x] - a, eb = pre_b + sb[threadIdx.x] - b;
#pragma unroll
    for (unsigned j = 0; j < SCAN_PER; j++)
        if (base + j < n) {
            offsets[base + j] = ea + va[j];
            if (cursor) cursor[base + j] = ea + va[j];
            seg_off[base + j] = eb + vb[j];
        }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == SCAN_T - 1) {
        offsets[n] = pre_a + sa[threadIdx.x];
        seg_off[n] = pre_b + sb[threadIdx.x];
        misc[0]    = pre_a + sa[threadIdx.x];
        misc[1]    = pre_b + sb[threadIdx.x];
    }
    // (3) the owning bucket of every segment and the histogram of segment lengths (the accumulation issues segments
    // longest first: k_seg_scatter).  A bucket's segments are nseg - 1 full ones and a last one with the remainder.
    // (Was a kernel of its own that found the bucket of every segment by a 20-step binary search.)
    __shared__ uint32_t big_n, big_b[64], big_s0[64], big_ns[64]; // buckets of this block with many segments
    if (threadIdx.x == 0) big_n = 0;
    k16_lds_sync();
#pragma unroll 1
    for (unsigned j = 0; j < SCAN_PER; j++) {
        const uint32_t nseg = base + j < n ? ns[j] : 0u;
        if (nseg) {
            const uint32_t s0 = eb + vb[j];
            uint32_t       slot = 64;
            if (nseg > 32) slot = atomicAdd(&big_n, 1u);
            if (slot < 64) { // skewed scalars: ~19 k segments in ONE bucket (witness MSMs) -- filled by the whole block below
                big_b[slot]  = base + j;
                big_s0[slot] = s0;
                big_ns[slot] = nseg;
            } else {
                for (uint32_t k = 0; k < nseg; k++) seg_bucket[s0 + k] = base + j;
            }
            if (nseg > 1) atomicAdd(&lh[seg], nseg - 1);
            atomicAdd(&lh[xs[j] - (nseg - 1) * seg], 1u);
        }
    }
    k16_lds_sync();
    {
        const uint32_t nbig = min(big_n, 64u);
        for (uint32_t q = 0; q < nbig; q++) {
            const uint32_t bb = big_b[q], s0 = big_s0[q], nsq = big_ns[q];
            for (uint32_t k = threadIdx.x; k < nsq; k += SCAN_T) seg_bucket[s0 + k] = bb;
        }
    }
    k16_lds_sync();
    for (unsigned i = threadIdx.x; i <= seg; i += SCAN_T)
        if (lh[i]) atomicAdd(&seg_hist[i], lh[i]);
    // (4) size classes of the fold (wave-uniform trip count: every lane walks its 16 slots)
#pragma unroll 1
    for (unsigned j = 0; j < SCAN_PER; j++) {
        const uint32_t bkt  = base + j;
        const uint32_t nseg = bkt < n ? ns[j] : 0u;
        wave_append(nseg > FOLD_SERIAL && nseg <= FOLD_SMALL, bkt, tree_list, misc + 4, med_cap);
        // more giant buckets than the giant list holds (heavily repeated digits at large n: 2^24 points over 16 distinct
        // values per window): the overflow goes to the medium list, whose fold handles any segment count with its
        // strided loop (one workgroup per bucket instead of 64) -- slower for those buckets, never wrong
        const bool giant  = nseg > FOLD_GIANT;
        const bool stored = wave_append(giant, bkt, giant_list, misc + 3, GIANT_CAP);
        wave_append((nseg > FOLD_SMALL && !giant) || (giant && !stored), bkt, med_list, misc + 2, med_cap);
    }
}

// ------------------------------------------------------------------------------------------
// K2: bucket accumulation.  One lane per segment (<= SEG consecutive entries of one bucket's
// index list).  The accumulator stays in registers; points are gathered by index (64 B / 128 B
// rows, served from L2 / Infinity Cache: the table is read W times per MSM).
// ------------------------------------------------------------------------------------------
// Arithmetic "engines": what a kernel needs to know about the group it accumulates in.
//   Row   element type of the base table in HBM          AffR  the same point in registers
//   Pt    XYZZ accumulator (registers and workspace)
// EngCanon<F>: the canonical 8x32-bit Montgomery field (G2 today).  Eng9: G1 over the unsaturated
// radix-2^29 field (bn254_fq9.h); its table rows are 64-byte packed R'-domain coordinates produced
// once per table by k_convert_bases.
template <class F>
struct EngCanon {
    typedef Aff<F>  Row;
    typedef Aff<F>  AffR;
    typedef Xyzz<F> Pt;
    typedef Xyzz<F> HostPt;
    static __device__ __forceinline__ AffR load_row(const Row* __restrict__ p) { return load_vec(p); }
    static __device__ __forceinline__ AffR negate(const AffR& a) { return pneg(a); } // (0,0) stays (0,0): -0 = 0 canonically
    static __device__ __forceinline__ Pt   zero() { return Xyzz<F>::zero(); }
    static __device__ __forceinline__ Pt   madd(const Pt& a, const AffR& b) { return padd_mixed(a, b); }
    static __device__ __forceinline__ Pt   add(const Pt& a, const Pt& b) { return padd(a, b); }
    static __device__ __forceinline__ Pt   neg(const Pt& a) { return pneg(a); }
    // the accumulator of the bucket accumulation's hot loop (an engine may keep it in a cheaper form than Pt: Eng9)
    typedef Pt Acc;
    static __device__ __forceinline__ Acc  acc_zero() { return zero(); }
    static __device__ __forceinline__ Acc  acc_from(const Pt& p) { return p; }
    static __device__ __forceinline__ void acc_madd(Acc& a, const AffR& row, uint32_t sign) { a = madd(a, sign ? negate(row) : row); }
    static __device__ __forceinline__ Pt   acc_finish(const Acc& a) { return a; }
    // lanes per point and row type of the bucket ACCUMULATION (2 / a lane's half for the G2 lane pairs)
    static constexpr unsigned ALPP = 1;
    typedef AffR ARow;
    static __device__ __forceinline__ ARow aload_row(const Row* __restrict__ p) { return load_row(p); }
    static __device__ __forceinline__ void acc_store(Pt* __restrict__ p, const Acc& a) { store_vec(p, acc_finish(a)); }
    // the latency-bound reductions (fold / weighted-sum kernels): lanes per point and the point type a lane holds there
    static constexpr unsigned LPP = 1;
    typedef Pt TPt;
    static __device__ __forceinline__ TPt  tzero() { return zero(); }
    static __device__ __forceinline__ TPt  tadd(const TPt& a, const TPt& b) { return add(a, b); }
    static __device__ __forceinline__ TPt  tload(const Pt* __restrict__ p) { return load_vec(p); }
    static __device__ __forceinline__ void tstore(Pt* __restrict__ p, const TPt& v) { store_vec(p, v); }
    static constexpr bool                  needs_convert = false;
    static constexpr bool                  has_aff_add   = false;
    static constexpr int                   ACC_MIN_WAVES = 1;
};
struct Eng9 {
    typedef Aff<Fq> Row;
    typedef Aff9    AffR;
    typedef Xyzz9   Pt;
    static __device__ __forceinline__ AffR load_row(const Row* __restrict__ p)
    {
        Aff<Fq> w = load_vec(p);
        return Aff9{fq9_unpack(w.x.v), fq9_unpack(w.y.v)};
    }
    // -(x, y) = (x, 2p - y), y < 2p -> <= 2p; the (0,0) row must keep its exact zero limbs (that is how it is recognised)
    static __device__ __forceinline__ AffR negate(const AffR& a)
    {
        if (a.is_zero()) return a;
        return Aff9{a.x, fsub9<2>(fq9_zero(), a.y)}; // 2p - y < 2p: y != 0 for a point on the curve
    }
    static __device__ __forceinline__ Pt zero() { return Xyzz9::zero(); }
    static __device__ __forceinline__ Pt madd(const Pt& a, const AffR& b) { return padd_mixed9(a, b); }
    static __device__ __forceinline__ Pt add_aff(const AffR& a, const AffR& b) { return padd_aff_aff9(a, b); }
    static constexpr bool                has_aff_add = true;
#ifndef K16_G1_ACC_MIN_WAVES
#define K16_G1_ACC_MIN_WAVES 3
#endif
    static constexpr int                 ACC_MIN_WAVES = K16_G1_ACC_MIN_WAVES; // waves per SIMD the accumulation is compiled for (3: at most 168 registers)
    static __device__ __forceinline__ Pt add(const Pt& a, const Pt& b) { return padd9(a, b); }
    static __device__ __forceinline__ Pt neg(const Pt& a) { return Xyzz9{a.x, fsub9<4>(fq9_zero(), a.y), a.zz, a.zzz}; } // Y < 4p -> 4p - Y < 4p
    // hot-loop accumulator: W = +-Y with a flag, lazy subtractions (bn254_fq9.h, acc9_madd); K16_ACC_OLD_FORMULAS: round 4's
#ifdef K16_ACC_OLD_FORMULAS
    typedef Pt Acc;
    static __device__ __forceinline__ Acc  acc_zero() { return zero(); }
    static __device__ __forceinline__ Acc  acc_from(const Pt& p) { return p; }
    static __device__ __forceinline__ void acc_madd(Acc& a, const AffR& row, uint32_t sign) { a = madd(a, sign ? negate(row) : row); }
    static __device__ __forceinline__ Pt   acc_finish(const Acc& a) { return a; }
#else
    typedef Acc9 Acc;
    static __device__ __forceinline__ Acc  acc_zero() { return Acc9::zero(); }
    static __device__ __forceinline__ Acc  acc_from(const Pt& p) { return Acc9::from_xyzz(p); }
    static __device__ __forceinline__ void acc_madd(Acc& a, const AffR& row, uint32_t sign) { acc9_madd(a, row, sign); }
    static __device__ __forceinline__ Pt   acc_finish(const Acc& a) { return a.to_xyzz(); }
#endif
    // lanes per point and row type of the bucket ACCUMULATION (2 / a lane's half for the G2 lane pairs)
    static constexpr unsigned ALPP = 1;
    typedef AffR ARow;
    static __device__ __forceinline__ ARow aload_row(const Row* __restrict__ p) { return load_row(p); }
    static __device__ __forceinline__ void acc_store(Pt* __restrict__ p, const Acc& a) { store_vec(p, acc_finish(a)); }
    // the latency-bound reductions (fold / weighted-sum kernels): lanes per point and the point type a lane holds there
    static constexpr unsigned LPP = 1;
    typedef Pt TPt;
    static __device__ __forceinline__ TPt  tzero() { return zero(); }
    static __device__ __forceinline__ TPt  tadd(const TPt& a, const TPt& b) { return add(a, b); }
    static __device__ __forceinline__ TPt  tload(const Pt* __restrict__ p) { return load_vec(p); }
    static __device__ __forceinline__ void tstore(Pt* __restrict__ p, const TPt& v) { store_vec(p, v); }
    static constexpr bool                needs_convert = true;
};

// G2 over Fq2n (Fq2 on the radix-2^29 field, components kept < 2p by fred9): rows are 128-byte packed
// R'-domain coordinates; the generic XYZZ formulas of bn254_curve.h are used as they are.
struct Eng2n {
    typedef Aff<Fq2>   Row;
    typedef Aff<Fq2n>  AffR;
    typedef Xyzz<Fq2n> Pt;
    static __device__ __forceinline__ AffR load_row(const Row* __restrict__ p)
    {
        Aff<Fq2> w = load_vec(p);
        return AffR{Fq2n{fq9_unpack(w.x.a.v), fq9_unpack(w.x.b.v)}, Fq2n{fq9_unpack(w.y.a.v), fq9_unpack(w.y.b.v)}};
    }
    static __device__ __forceinline__ AffR negate(const AffR& a)
    {
        if (a.is_zero()) return a;
        return AffR{a.x, fneg(a.y)};
    }
    static __device__ __forceinline__ Pt zero() { return Xyzz<Fq2n>::zero(); }
    static __device__ __forceinline__ Pt madd(const Pt& a, const AffR& b) { return padd_mixed(a, b); }
    static __device__ __forceinline__ Pt add(const Pt& a, const Pt& b) { return padd(a, b); }
    static __device__ __forceinline__ Pt neg(const Pt& a) { return pneg(a); }
#if defined(K16_G2_NO_PAIRS) || defined(K16_G2_NO_PAIR_ACC)
    typedef Pt Acc;
    static __device__ __forceinline__ Acc  acc_zero() { return zero(); }
    static __device__ __forceinline__ Acc  acc_from(const Pt& p) { return p; }
    static __device__ __forceinline__ void acc_madd(Acc& a, const AffR& row, uint32_t sign) { a = madd(a, sign ? negate(row) : row); }
    static __device__ __forceinline__ Pt   acc_finish(const Acc& a) { return a; }
    // lanes per point and row type of the bucket ACCUMULATION (2 / a lane's half for the G2 lane pairs)
    static constexpr unsigned ALPP = 1;
    typedef AffR ARow;
    static __device__ __forceinline__ ARow aload_row(const Row* __restrict__ p) { return load_row(p); }
    static __device__ __forceinline__ void acc_store(Pt* __restrict__ p, const Acc& a) { store_vec(p, acc_finish(a)); }
#else
    // the bucket accumulation on LANE PAIRS as well: a G2 segment is a chain of 32 dependent mixed additions walked at a lone
    // wave's issue rate (the witness MSM's B2 accumulation is 1.0 ms of latency, not of work); a pair halves every link
    static constexpr unsigned ALPP = 2;
    typedef Aff<Fq2h>  ARow;
    typedef Xyzz<Fq2h> Acc;
    static __device__ __forceinline__ ARow aload_row(const Row* __restrict__ p)
    {
        const Fq* f = reinterpret_cast<const Fq*>(p) + (threadIdx.x & 1u); // x.a x.b y.a y.b, 32 packed bytes each
        const Fq  x = load_vec(f), y = load_vec(f + 2);
        return ARow{Fq2h{fq9_unpack(x.v)}, Fq2h{fq9_unpack(y.v)}};
    }
    static __device__ __forceinline__ Acc  acc_zero() { return Xyzz<Fq2h>::zero(); }
    // -(x, y) = (x, -y); a (0,0) row stays zero MODULO p, which is what Aff<Fq2h>::is_zero() tests
    static __device__ __forceinline__ void acc_madd(Acc& a, const ARow& row, uint32_t sign)
    {
        a = padd_mixed(a, sign ? ARow{row.x, fneg(row.y)} : row);
    }
    static __device__ __forceinline__ void acc_store(Pt* __restrict__ p, const Acc& a)
    {
        Fq9* f = reinterpret_cast<Fq9*>(p) + (threadIdx.x & 1u);
        f[0]   = a.x.v;
        f[2]   = a.y.v;
        f[4]   = a.zz.v;
        f[6]   = a.zzz.v;
    }
#endif
    // the latency-bound reductions run on LANE PAIRS (bn254_fq2pair.h): the even lane of a pair holds the real parts of the
    // point's four coordinates, the odd lane the imaginary parts -- half the dependent multiply-adds per addition and half the
    // registers of a lane that holds whole Fq2 values.  Points in memory keep the Xyzz<Fq2n> layout (x.a x.b y.a y.b zz.a ...).
#ifndef K16_G2_NO_PAIRS
    static constexpr unsigned LPP = 2;
    typedef Xyzz<Fq2h> TPt;
    static __device__ __forceinline__ TPt tzero() { return Xyzz<Fq2h>::zero(); }
    static __device__ __forceinline__ TPt tadd(const TPt& a, const TPt& b) { return padd(a, b); }
    static __device__ __forceinline__ TPt tload(const Pt* __restrict__ p)
    {
        const Fq9* f = reinterpret_cast<const Fq9*>(p) + (threadIdx.x & 1u);
        return TPt{Fq2h{f[0]}, Fq2h{f[2]}, Fq2h{f[4]}, Fq2h{f[6]}};
    }
    static __device__ __forceinline__ void tstore(Pt* __restrict__ p, const TPt& v)
    {
        Fq9* f = reinterpret_cast<Fq9*>(p) + (threadIdx.x & 1u);
        f[0]   = v.x.v;
        f[2]   = v.y.v;
        f[4]   = v.zz.v;
        f[6]   = v.zzz.v;
    }
#else
    // the latency-bound reductions (fold / weighted-sum kernels): lanes per point and the point type a lane holds there
    static constexpr unsigned LPP = 1;
    typedef Pt TPt;
    static __device__ __forceinline__ TPt  tzero() { return zero(); }
    static __device__ __forceinline__ TPt  tadd(const TPt& a, const TPt& b) { return add(a, b); }
    static __device__ __forceinline__ TPt  tload(const Pt* __restrict__ p) { return load_vec(p); }
    static __device__ __forceinline__ void tstore(Pt* __restrict__ p, const TPt& v) { store_vec(p, v); }
#endif
    static constexpr bool                needs_convert = true;
    static constexpr bool                has_aff_add   = false;
#ifndef K16_G2_ACC_MIN_WAVES
#define K16_G2_ACC_MIN_WAVES 1
#endif
    static constexpr int                 ACC_MIN_WAVES = K16_G2_ACC_MIN_WAVES; // (lab: 2 = at most 256 registers, two waves per SIMD)
};
__global__ void __launch_bounds__(256) k_convert_bases_g2(const Aff<Fq2>* __restrict__ in, Aff<Fq2>* __restrict__ out,
                                                          uint64_t n)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Aff<Fq2> a = load_vec(&in[i]);
    Aff<Fq2> o;
    fq9_pack(o.x.a.v, fq9_from_fq(a.x.a));
    fq9_pack(o.x.b.v, fq9_from_fq(a.x.b));
    fq9_pack(o.y.a.v, fq9_from_fq(a.y.a));
    fq9_pack(o.y.b.v, fq9_from_fq(a.y.b));
    store_vec(&out[i], o);
}

// canonical zkey-format G1 table -> packed R'-domain rows (x*R', y*R' < 2p; (0,0) stays (0,0))
__global__ void __launch_bounds__(256) k_convert_bases(const Aff<Fq>* __restrict__ in, Aff<Fq>* __restrict__ out,
                                                       uint64_t n)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Aff<Fq> a = load_vec(&in[i]);
    Aff9    c = aff9_from_canonical(a);
    Aff<Fq> o;
    fq9_pack(o.x.v, c.x);
    fq9_pack(o.y.v, c.y);
    store_vec(&out[i], o);
}

// largest b with seg_off[b] <= s  (seg_off has nb+1 entries, non-decreasing, seg_off[nb] = total)
__device__ __forceinline__ uint32_t find_bucket(const uint32_t* __restrict__ seg_off, uint32_t nb, uint32_t s)
{
    uint32_t lo = 0, hi = nb; // invariant: seg_off[lo] <= s < seg_off[hi]
    while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (seg_off[mid] <= s)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// Segment scheduling: segments are issued in order of decreasing length so that the 64 lanes of a
// wave run (nearly) the same number of mixed adds -- bucket sizes are Poisson-distributed and an
// unsorted assignment leaves ~40 % of the lanes idle behind the longest bucket of the wave.
// Counting sort by length (1..SEG): the histogram and seg_bucket[] (the owning bucket of every segment) come from
// k_scan2_apply, the scatter is k_seg_scatter.
__device__ __forceinline__ uint32_t seg_length(const uint32_t* __restrict__ off, const uint32_t* __restrict__ seg_off,
                                               uint32_t b, uint32_t s, uint32_t seg)
{
    uint32_t k  = s - seg_off[b];
    uint32_t lo = off[b] + k * seg;
    uint32_t hi = min(lo + seg, off[b + 1]);
    return hi - lo;
}
// Segments are written in order of decreasing length: position = start[len] + rank among the segments of that length,
// start[len] = number of segments strictly longer than len.  Every workgroup derives start[] from the length histogram
// itself (a 1025-entry suffix sum in LDS) -- it used to be a single-wave kernel of its own in every lane's chain.
// Every workgroup owns a CONTIGUOUS range of segments (SEG_PER_THREAD per lane): it histograms the range's lengths in LDS,
// reserves its slice of every length class with ONE global atomic per class, and then ranks its segments inside the
// slices.  (Round 2: a 256-segment tile per trip, i.e. 2048 workgroups x ~40 classes of atomics onto the same ~80 cursor
// words -- 55 us for the H sort's 550 k segments, most of it waiting on those hot addresses.)
constexpr unsigned SEG_PER_THREAD = 8;
__global__ void __launch_bounds__(256) k_seg_scatter(const uint32_t* __restrict__ off, const uint32_t* __restrict__ seg_off,
                                                     const uint32_t* __restrict__ total_segs,
                                                     const uint32_t* __restrict__ seg_bucket,
                                                     const uint32_t* __restrict__ hist, uint32_t* __restrict__ cursor,
                                                     uint32_t* __restrict__ order, uint32_t seg)
{
    k16_short_kernel_prio();
    __shared__ uint32_t h[MAX_SEG + 1];
    __shared__ uint32_t base[MAX_SEG + 1];
    __shared__ uint32_t start[MAX_SEG + 1];
    __shared__ uint32_t sh[256];
    {
        // reversed index r = seg - len: start[len] = sum_{r' < r} hist[seg - r']
        const unsigned per = (seg + 1 + 255) / 256;
        uint32_t       sum = 0;
        for (unsigned j = 0; j < per; j++) {
            unsigned r = threadIdx.x * per + j;
            if (r <= seg) sum += hist[seg - r];
        }
        sh[threadIdx.x] = sum;
        k16_lds_sync();
        for (unsigned o = 1; o < 256; o <<= 1) {
            uint32_t t = threadIdx.x >= o ? sh[threadIdx.x - o] : 0u;
            k16_lds_sync();
            sh[threadIdx.x] += t;
            k16_lds_sync();
        }
        uint32_t run = sh[threadIdx.x] - sum;
        for (unsigned j = 0; j < per; j++) {
            unsigned r = threadIdx.x * per + j;
            if (r <= seg) {
                start[seg - r] = run;
                run += hist[seg - r];
            }
        }
    }
    for (unsigned i = threadIdx.x; i <= seg; i += blockDim.x) h[i] = 0;
    k16_lds_sync();
    const uint32_t nseg  = *total_segs;
    const uint32_t chunk = 256 * SEG_PER_THREAD;
    for (uint32_t c0 = blockIdx.x * chunk; c0 < nseg; c0 += gridDim.x * chunk) { // (one trip with the launch's grid)
        uint32_t len[SEG_PER_THREAD], rank[SEG_PER_THREAD];
#pragma unroll
        for (unsigned k = 0; k < SEG_PER_THREAD; k++) {
            const uint32_t s = c0 + k * 256 + threadIdx.x;
            len[k]           = s < nseg ? seg_length(off, seg_off, seg_bucket[s], s, seg) : 0xffffffffu;
        }
#pragma unroll
        for (unsigned k = 0; k < SEG_PER_THREAD; k++) rank[k] = len[k] != 0xffffffffu ? atomicAdd(&h[len[k]], 1u) : 0u;
        k16_lds_sync();
        for (unsigned i = threadIdx.x; i <= seg; i += blockDim.x) {
            if (h[i]) base[i] = start[i] + atomicAdd(&cursor[i], h[i]);
        }
        k16_lds_sync();
#pragma unroll
        for (unsigned k = 0; k < SEG_PER_THREAD; k++)
            if (len[k] != 0xffffffffu) order[base[len[k]] + rank[k]] = c0 + k * 256 + threadIdx.x;
        k16_lds_sync();
        for (unsigned i = threadIdx.x; i <= seg; i += blockDim.x) h[i] = 0;
        k16_lds_sync();
    }
}

template <class E>
__global__ void __launch_bounds__(128 * E::ALPP, E::ACC_MIN_WAVES) k_accumulate(const typename E::Row* __restrict__ bases,
                                                    const uint32_t* __restrict__ sorted,
                                                    const uint32_t* __restrict__ off,
                                                    const uint32_t* __restrict__ seg_off,
                                                    const uint32_t* __restrict__ seg_bucket,
                                                    const uint32_t* __restrict__ order,
                                                    const uint32_t* __restrict__ total_segs,
                                                    typename E::Pt* __restrict__ partial, uint32_t seg)
{
    k16_acc_prio<E>();
    const uint32_t nseg = *total_segs;
    // (E::ALPP lanes per segment: 1, or the G2 lane pairs of bn254_fq2pair.h -- `t` is the LOGICAL lane)
    for (uint32_t t = (blockIdx.x * blockDim.x + threadIdx.x) / E::ALPP; t < nseg; t += gridDim.x * blockDim.x / E::ALPP) {
        uint32_t s  = order[t];
        uint32_t b  = seg_bucket[s];
        uint32_t k  = s - seg_off[b];
        uint32_t lo = off[b] + k * seg;
        uint32_t hi = min(lo + seg, off[b + 1]);
        // an entry is sign << 31 | row: the row is gathered as it lies in the table, the sign (signed digits, see
        // for_signed_digits) goes into the addition (E::acc_madd)
        auto gather = [&](uint32_t e) -> typename E::ARow { return E::aload_row(&bases[e & 0x7fffffffu]); };
        typename E::Acc  acc = E::acc_zero();
        uint32_t         en  = sorted[lo];
        typename E::ARow nxt = gather(en); // lo < hi always: a segment is never empty
        uint32_t         j   = lo;
        if constexpr (E::has_aff_add) {
            // the first two rows are both affine: 6 instead of 10 multiplications (segments are issued longest
            // first, so the lanes of a wave take this branch together)
            if (lo + 1 < hi) {
                const uint32_t   e2    = sorted[lo + 1];
                typename E::AffR first = (en >> 31) ? E::negate(nxt) : nxt, second = gather(e2);
                if (e2 >> 31) second = E::negate(second);
                if (lo + 2 < hi) {
                    en  = sorted[lo + 2];
                    nxt = gather(en);
                }
                acc = E::acc_from(E::add_aff(first, second));
                j   = lo + 2;
            }
        }
        for (; j < hi; j++) {
            typename E::ARow cur = nxt;
            const uint32_t   ec  = en;
            if (j + 1 < hi) {
                en  = sorted[j + 1];
                nxt = gather(en); // gather for the next add flies during this one
            }
            E::acc_madd(acc, cur, ec >> 31);
        }
        E::acc_store(&partial[s], acc);
    }
}

// The same with a zero-row mask (bit r set: table row r is (0,0)) for a table that READS another table's bucket sort: the
// prover's B1 / B2, half of whose rows are (0,0) in a circuit whose wires mostly sit on one side of a constraint, share A's
// sort.  Adding a (0,0) row returns the accumulator unchanged (curve.cpp:185-250), but the lane sits out a whole addition
// of its wave; here a lane steps over its masked entries (one bit each, L2-resident) BEFORE the wave's next addition, so a
// wave runs as many additions as its busiest lane has unmasked entries: ~23 instead of 32 at 50 % zeros.  Same sums.
template <class E>
__global__ void __launch_bounds__(128 * E::ALPP, E::ACC_MIN_WAVES) k_accumulate_skip(const typename E::Row* __restrict__ bases,
                                                    const uint32_t* __restrict__ sorted,
                                                    const uint32_t* __restrict__ off,
                                                    const uint32_t* __restrict__ seg_off,
                                                    const uint32_t* __restrict__ seg_bucket,
                                                    const uint32_t* __restrict__ order,
                                                    const uint32_t* __restrict__ total_segs,
                                                    typename E::Pt* __restrict__ partial, uint32_t seg,
                                                    const uint64_t* __restrict__ skip)
{
    k16_acc_prio<E>();
    const uint32_t nseg = *total_segs;
    for (uint32_t t = (blockIdx.x * blockDim.x + threadIdx.x) / E::ALPP; t < nseg; t += gridDim.x * blockDim.x / E::ALPP) {
        uint32_t s  = order[t];
        uint32_t b  = seg_bucket[s];
        uint32_t k  = s - seg_off[b];
        uint32_t lo = off[b] + k * seg;
        uint32_t hi = min(lo + seg, off[b + 1]);
        auto gather = [&](uint32_t e) -> typename E::ARow { return E::aload_row(&bases[e & 0x7fffffffu]); };
        // first unmasked entry at or behind j (hi: none); *e receives it
        auto next_live = [&](uint32_t j, uint32_t* e) -> uint32_t {
            while (j < hi) {
                const uint32_t v = sorted[j], row = v & 0x7fffffffu;
                if (!((skip[row >> 6] >> (row & 63u)) & 1ull)) {
                    *e = v;
                    return j;
                }
                j++;
            }
            return hi;
        };
        typename E::Acc  acc = E::acc_zero();
        typename E::ARow nxt;
        uint32_t         e = 0;
        uint32_t         j = next_live(lo, &e);
        if (j < hi) nxt = gather(e);
        while (j < hi) {
            typename E::ARow cur = nxt;
            const uint32_t   ec  = e;
            const uint32_t   j2  = next_live(j + 1, &e);
            if (j2 < hi) nxt = gather(e); // gather for the next add flies during this one
            E::acc_madd(acc, cur, ec >> 31);
            j = j2;
        }
        E::acc_store(&partial[s], acc);
    }
}

// 16-lane shuffle of a whole point (tree fold of buckets with 5..16 segments)
template <class T>
__device__ __forceinline__ T shfl_down_vec(const T& v, unsigned delta, int width = 16)
{
    static_assert(sizeof(T) % 4 == 0, "dword granularity");
    T               r;
    const uint32_t* s = reinterpret_cast<const uint32_t*>(&v);
    uint32_t*       d = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 4; i++) d[i] = (uint32_t)__shfl_down((int)s[i], delta, width);
    return r;
}

// One launch folds every size class (the lists come from k_scan2_apply); the role of a workgroup follows from its index:
//   [0, nS)            serial: one lane per bucket with 2 .. FOLD_SERIAL segments (grid-stride over all buckets)
//   [nS, nS+nT)        tree:   16 lanes per bucket with <= 16 segments (e.g. the 255 byte-valued buckets of a witness
//                              MSM, ~14 segments each): one partial per lane, 4-step shuffle tree
//   [.., +nB)          big:    one workgroup per bucket, strided sums + LDS tree
//   [.., +GIANT_BLOCKS) giant: block k sums the partials lo + k*256 + t (+ multiples of GIANT_BLOCKS*256) of every giant
//                              bucket into scratch[g * GIANT_BLOCKS + k]; k_fold_giant_b finishes them
// (Four kernels before; with uniform scalars three of them find empty lists, but each still cost a slot in the chain.)
// (E::LPP lanes per point: 1, or 2 for the G2 lane pairs of bn254_fq2pair.h -- `t` below is the LOGICAL lane, a point's lanes
// are adjacent, every lane of a point takes the same branches; LDS trees index by the physical lane, so partner lanes pair up)
template <class E>
__global__ void __launch_bounds__(256 * E::LPP) k_fold_all(const uint32_t* __restrict__ seg_off, uint32_t nb,
                                                  const uint32_t* __restrict__ tree_list, const uint32_t* __restrict__ med_list,
                                                  const uint32_t* __restrict__ giant_list, const uint32_t* __restrict__ misc,
                                                  uint32_t cap, typename E::Pt* __restrict__ partial,
                                                  typename E::Pt* __restrict__ scratch, uint32_t nS, uint32_t nT, uint32_t nB)
{
    k16_short_kernel_prio();
    constexpr unsigned LPP = E::LPP;
    extern __shared__ uint4 lds_raw[];
    typename E::TPt*        lds = reinterpret_cast<typename E::TPt*>(lds_raw);
    const unsigned          t   = threadIdx.x / LPP; // 0 .. 255
    if (blockIdx.x < nS) {
        for (uint32_t b = blockIdx.x * 256 + t; b < nb; b += nS * 256) {
            uint32_t lo = seg_off[b], hi = seg_off[b + 1];
            if (hi - lo < 2 || hi - lo > FOLD_SERIAL) continue;
            typename E::TPt acc = E::tload(&partial[lo]);
#pragma clang loop unroll(disable)
            for (uint32_t j = lo + 1; j < hi; j++) acc = E::tadd(acc, E::tload(&partial[j]));
            E::tstore(&partial[lo], acc);
        }
    } else if (blockIdx.x < nS + nT) {
        const uint32_t blk = blockIdx.x - nS;
        const uint32_t nt  = min(misc[4], cap);
        const uint32_t sub = t >> 4, l = t & 15; // 16 buckets per workgroup, 4 per wave (2 per wave on lane pairs)
        for (uint32_t g0 = blk * 16; g0 < nt; g0 += nT * 16) {       // wave-uniform trip count
            const uint32_t g  = g0 + sub;
            uint32_t       lo = 0, hi = 0;
            if (g < nt) {
                uint32_t b = tree_list[g];
                lo = seg_off[b];
                hi = seg_off[b + 1];
            }
            typename E::TPt acc = E::tzero();
            if (lo + l < hi) acc = E::tload(&partial[lo + l]);
#pragma clang loop unroll(disable)
            for (unsigned d = 8; d > 0; d >>= 1) {
                typename E::TPt o = shfl_down_vec(acc, d * LPP, 16 * LPP);
                acc = E::tadd(acc, o);
            }
            if (l == 0 && g < nt) E::tstore(&partial[lo], acc);
        }
    } else if (blockIdx.x < nS + nT + nB) {
        const uint32_t blk  = blockIdx.x - nS - nT;
        const uint32_t nmed = min(misc[2], cap);
        for (uint32_t bi = blk; bi < nmed; bi += nB) {
            uint32_t       b  = med_list[bi];
            uint32_t       lo = seg_off[b], hi = seg_off[b + 1];
            typename E::TPt acc = E::tzero();
#pragma clang loop unroll(disable)
            for (uint32_t j = lo + t; j < hi; j += 256) acc = E::tadd(acc, E::tload(&partial[j]));
            lds[threadIdx.x] = acc;
            k16_lds_sync();
#pragma clang loop unroll(disable)
            for (unsigned o = 128; o > 0; o >>= 1) {
                if (t < o) {
                    typename E::TPt a = lds[threadIdx.x], c = lds[threadIdx.x + o * LPP];
                    lds[threadIdx.x] = E::tadd(a, c);
                }
                k16_lds_sync();
            }
            if (t == 0) E::tstore(&partial[lo], lds[threadIdx.x]);
            k16_lds_sync();
        }
    } else {
        const uint32_t blk = blockIdx.x - nS - nT - nB; // 0 .. GIANT_BLOCKS-1
        const uint32_t ng  = min(misc[3], GIANT_CAP);
        for (uint32_t g = 0; g < ng; g++) {
            uint32_t       b  = giant_list[g];
            uint32_t       lo = seg_off[b], hi = seg_off[b + 1];
            typename E::TPt acc = E::tzero();
#pragma clang loop unroll(disable)
            for (uint32_t j = lo + blk * 256 + t; j < hi; j += GIANT_BLOCKS * 256)
                acc = E::tadd(acc, E::tload(&partial[j]));
            lds[threadIdx.x] = acc;
            k16_lds_sync();
#pragma clang loop unroll(disable)
            for (unsigned o = 128; o > 0; o >>= 1) {
                if (t < o) {
                    typename E::TPt a = lds[threadIdx.x], c = lds[threadIdx.x + o * LPP];
                    lds[threadIdx.x] = E::tadd(a, c);
                }
                k16_lds_sync();
            }
            if (t == 0) E::tstore(&scratch[g * GIANT_BLOCKS + blk], lds[threadIdx.x]);
            k16_lds_sync();
        }
    }
}
template <class E>
__global__ void __launch_bounds__(64 * E::LPP) k_fold_giant_b(const uint32_t* __restrict__ seg_off,
                                                     const uint32_t* __restrict__ giant_list,
                                                     const uint32_t* __restrict__ giant_count,
                                                     typename E::Pt* __restrict__ partial,
                                                     const typename E::Pt* __restrict__ scratch)
{
    k16_short_kernel_prio();
    constexpr unsigned LPP = E::LPP;
    extern __shared__ uint4 lds_raw[];
    typename E::TPt*        lds = reinterpret_cast<typename E::TPt*>(lds_raw);
    const unsigned          t   = threadIdx.x / LPP; // 0 .. 63
    uint32_t                ng  = min(*giant_count, GIANT_CAP);
    for (uint32_t g = blockIdx.x; g < ng; g += gridDim.x) {
        lds[threadIdx.x] = E::tload(&scratch[g * GIANT_BLOCKS + t]);
        k16_lds_sync();
        for (unsigned o = 32; o > 0; o >>= 1) {
            if (t < o) {
                typename E::TPt a = lds[threadIdx.x], c = lds[threadIdx.x + o * LPP];
                lds[threadIdx.x] = E::tadd(a, c);
            }
            k16_lds_sync();
        }
        if (t == 0) E::tstore(&partial[seg_off[giant_list[g]]], lds[threadIdx.x]);
        k16_lds_sync();
    }
}

// ------------------------------------------------------------------------------------------
// K4: per window, sum_d d*B_d, without long serial chains of EC additions.
//   pairing  signed digits: X_i = B[i] - B[2^c - i] for the magnitudes i = 1 .. 2^(c-1) (see for_signed_digits)
//   level 1  lane (w,u) owns the slots i' = u*M .. u*M+M-1 (M <= 8, magnitude i = i' + 1):
//              S[w][u] = sum_j X[u*M+j]        G[w][u] = sum_j j*X[u*M+j]      (running sums, 2M adds)
//            so that   sum_i i*X_i = sum_u G[w][u] + M * sum_u u*S[w][u] + sum_u S[w][u]
//   level 2  sum_u u*S[u] = sum_b 2^b * (sum over u with bit b set of S[u]):  one workgroup per
//            (window, bit) does a strided partial sum per lane and an LDS tree; one more workgroup
//            per window sums G.  All of it is plain (unweighted) summation => log depth.
//   host     window value = T[w][nbits] + T[w][nbits+1] + M * sum_b 2^b T[w][b], then Horner over the windows.
// Empty buckets are infinity; buckets are read through (seg_off, partial).
// ------------------------------------------------------------------------------------------
// whole-point exchange between the two lanes of a pair (lane ^ 1)
template <class T>
__device__ __forceinline__ T shfl_xor1_vec(const T& v, int dist = 1)
{
    static_assert(sizeof(T) % 4 == 0, "dword granularity");
    T               r;
    const uint32_t* s = reinterpret_cast<const uint32_t*>(&v);
    uint32_t*       d = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 4; i++) d[i] = (uint32_t)__shfl_xor((int)s[i], dist);
    return r;
}

// Level 1 on LANE PAIRS: the two running sums of a slot group (S = sum X_j, G = sum j X_j) are two dependent chains of M
// additions each -- `acc += running; running += X_j`.  One lane would walk 2M additions holding three points (254 VGPRs:
// two waves per SIMD); here lane A of a pair does `running += X_j` and lane B, one step behind, `acc += running`, which it
// receives from A by a cross-lane shuffle before A's update: M additions per lane, two points live (~160 VGPRs), twice
// the lanes.  Same sums, same order of additions per chain.
template <class E, bool PREFETCH = false>
__global__ void __launch_bounds__(64 * E::LPP) k_wsum_level1(uint32_t U, uint32_t W, uint32_t M, const uint32_t* __restrict__ seg_off,
                                                    unsigned c, uint32_t flat, const typename E::Pt* __restrict__ partial,
                                                    typename E::Pt* __restrict__ S_out, typename E::Pt* __restrict__ G_out)
{
    k16_short_kernel_prio();
    constexpr unsigned LPP = E::LPP;
    const uint32_t tid  = (blockIdx.x * blockDim.x + threadIdx.x) / LPP; // logical lane
    const uint32_t pair = tid >> 1;
    const bool     isB  = tid & 1u;
    if (pair >= W * U) return; // both lanes of a pair leave together
    const uint32_t w = pair / U, u = pair % U;
    typename E::TPt mine = E::tzero();
    // ordinary MSM: window w owns the buckets (w << (c-1)) + 0 .. 2^(c-1) - 1 (bucket = digit magnitude - 1).  Flat
    // (fixed-base) MSM: one bucket space 0 .. 2^(c-1) - 1, cut into W pseudo-windows of U*M magnitudes each (the host
    // adds the offsets w * U*M back).
    const uint32_t key_base = flat ? w * U * M : (w << (c - 1));
    // a (pseudo-)window without a single entry -- the carry window of every MSM whose scalars are below 2^255, the high
    // windows of witness scalars: nothing to add; its lanes leave at once instead of walking M empty buckets
    if (seg_off[key_base] == seg_off[key_base + U * M]) {
        E::tstore(isB ? &G_out[(size_t)w * U + u] : &S_out[(size_t)w * U + u], mine);
        return;
    }
    // (PREFETCH: lane A fetches bucket j - 1 while it adds bucket j -- the two dependent loads of a bucket, seg_off then the
    // partial sum, are otherwise exposed M times on a chip this kernel does not fill; 158 -> 126 us alone in round 2, dropped
    // then for a proof-level difference inside the noise, re-measured in round 4)
    auto fetch = [&](int j) -> typename E::TPt {
        const uint32_t key = key_base + u * M + (uint32_t)j;
        const uint32_t s0  = seg_off[key];
        typename E::TPt o  = E::tzero();
        if (seg_off[key + 1] != s0) o = E::tload(&partial[s0]);
        return o;
    };
    typename E::TPt nxt = E::tzero();
    if (PREFETCH && !isB) nxt = fetch((int)M - 1);
#pragma clang loop unroll(disable)
    for (int j = (int)M - 1; j >= 0; j--) {
        // slot i' = u*M + j stands for the digit magnitude i' + 1 (of its window or pseudo-window)
        typename E::TPt operand = shfl_xor1_vec(mine, (int)LPP); // B: A's running sum BEFORE this step's update
        if (!isB) {
            if (PREFETCH) {
                operand = nxt;
                if (j > 0) nxt = fetch(j - 1);
            } else {
                operand = fetch(j);
            }
        }
        mine = E::tadd(mine, operand);
    }
    E::tstore(isB ? &G_out[(size_t)w * U + u] : &S_out[(size_t)w * U + u], mine);
}

// block (w, j): j < nbits -> sum of S[w][u] over u with bit j set ; j == nbits -> sum of G[w][u] ;
// j == nbits + 1 -> sum of all S[w][u].
// Lane t owns the R = U / 256 values u = insert(k, p) of t, k = 0 .. R-1: the bits of k sit at positions p .. p+log2(R)-1
// of u, with p chosen so that bit j of u is a bit of k -- then EVERY lane has exactly R/2 of its values selected (chain
// R/2), instead of half of the lanes having all R and the other half none when bit j comes from the lane number.
template <class E>
__global__ void __launch_bounds__(256 * E::LPP) k_wsum_bits(const typename E::Pt* __restrict__ S, const typename E::Pt* __restrict__ G,
                                                   uint32_t U, uint32_t nbits, typename E::Pt* __restrict__ T)
{
    k16_short_kernel_prio();
    constexpr unsigned LPP = E::LPP;
    extern __shared__ uint4 lds_raw[];
    typename E::TPt*               lds = reinterpret_cast<typename E::TPt*>(lds_raw);
    const unsigned                 t   = threadIdx.x / LPP; // logical lane 0 .. 255
    const uint32_t          w = blockIdx.x / (nbits + 2), j = blockIdx.x % (nbits + 2);
    const typename E::Pt*          src = (j == nbits ? G : S) + (size_t)w * U;
    typename E::TPt                acc = E::tzero();
    if (U >= 512) {
        const uint32_t R  = U >> 8;            // values per lane (power of two, >= 2)
        uint32_t       rb = 0;
        while ((1u << rb) < R) rb++;
        const uint32_t p  = j < nbits ? (j + rb <= nbits ? j : nbits - rb) : 0u; // bit j of u lies inside k's field
        const uint32_t lo = t & ((1u << p) - 1u), hi = t >> p;
        // the selected values of a lane are known up front (bit j of u is a bit of k): the next one is fetched while the
        // current one is added (a lane's chain is R / 2 additions with an exposed load each otherwise)
        auto sel = [&](uint32_t k) -> bool { return !(j < nbits) || (((lo | (k << p) | (hi << (p + rb))) >> j) & 1u); };
        uint32_t k = 0;
        while (k < R && !sel(k)) k++;
        typename E::TPt nxt = E::tzero();
        if (k < R) nxt = E::tload(&src[lo | (k << p) | (hi << (p + rb))]);
#pragma clang loop unroll(disable)
        while (k < R) {
            typename E::TPt cur = nxt;
            uint32_t        k2  = k + 1;
            while (k2 < R && !sel(k2)) k2++;
            if (k2 < R) nxt = E::tload(&src[lo | (k2 << p) | (hi << (p + rb))]);
            acc = E::tadd(acc, cur);
            k   = k2;
        }
    } else {
        for (uint32_t u = t; u < U; u += 256) {
            if (j < nbits && !((u >> j) & 1)) continue;
            acc = E::tadd(acc, E::tload(&src[u]));
        }
    }
    lds[threadIdx.x] = acc;
    k16_lds_sync();
    for (unsigned o = 128; o > 0; o >>= 1) {
        if (t < o) {
            typename E::TPt a = lds[threadIdx.x], b = lds[threadIdx.x + o * LPP];
            lds[threadIdx.x] = E::tadd(a, b);
        }
        k16_lds_sync();
    }
    if (t == 0) E::tstore(&T[blockIdx.x], lds[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------
// Runs `body` (a sequence of launches / memsets / copies on `st`) eagerly, or -- with graphs on -- captures it the second
// time it is seen with this key and replays the executable graph from then on (ctx.h, graphs_on).
template <class Body>
int run_graph_section(k16_ctx* ctx, k16_ctx::Lane& L, hipStream_t st, const k16_ctx::Lane::GraphKey& key, Body body)
{
    if (!ctx->graphs_on) return body();
    if (L.graphs_gen != ctx->ws_gen) { // a workspace moved: every cached graph holds stale pointers
        for (auto& kv : L.graphs)
            if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
        L.graphs.clear();
        L.graphs_gen = ctx->ws_gen;
    }
    k16_ctx::Lane::GraphEntry& ge = L.graphs[key];
    if (ge.state == 2) {
        K16_HIP(ctx, hipGraphLaunch(ge.exec, st));
        return K16_OK;
    }
    if (ge.state == 0) { // first time: eager, so that every workspace is sized before anything is captured
        const uint64_t gen = ctx->ws_gen;
        int            rc  = body();
        if (!rc && gen == ctx->ws_gen) ge.state = 1; // (the map may have been cleared only at the next call)
        return rc;
    }
    if (ge.state < 0) return body();
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        ge.state = -1;
        return body();
    }
    ctx->capturing = true;
    int        rc  = body();
    hipGraph_t g   = nullptr;
    hipError_t e   = hipStreamEndCapture(st, &g);
    ctx->capturing = false;
    if (rc || e != hipSuccess || !g || hipGraphInstantiate(&ge.exec, g, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (g) (void)hipGraphDestroy(g);
        ge.exec  = nullptr;
        ge.state = -1;
        return rc ? rc : body(); // nothing was executed during the capture: run it now
    }
    (void)hipGraphDestroy(g);
    ge.state = 2;
    K16_HIP(ctx, hipGraphLaunch(ge.exec, st));
    return K16_OK;
}

// ------------------------------------------------------------------------------------------
// The bucket sort of one MSM as a sequence of launches on `st` (K1; everything the accumulation reads: sorted index
// lists, bucket offsets, segment offsets / owners / order, the fold's size classes).  A free function so that
// tools/lab/sortlab.hip can time and check it without compiling the EC kernels.
struct SortArgs {
    const void* d_scalars;
    uint64_t    n;
    unsigned    c, W;
    bool        flat;
    uint32_t    nb, seg, big_cap;
    size_t      max_segs, zr_words;
    uint32_t *  zr, *misc, *gcount, *gcursor, *seg_hist, *counts, *offsets, *cursor, *seg_off, *sorted, *scan_tmp, *big_list,
        *seg_bucket, *seg_order;
    const void* conv_in;
    void*       conv_out;
    const uint32_t* remap; // point k of the scalars is table row remap[k] (nullptr: k itself)
    const uint64_t* skip;  // bit i set: point i is left out (nullptr: none); k_part path only
    const void*     hs[3]; // non-null: d_scalars is still to be written -- scalar i = fromMontgomery(hs[0][i] * hs[1][i] - hs[2][i])
};
constexpr size_t SORT_GS = 8208; // >= NB1 + 1 for every partition config

template <class Tick>
int msm_sort_launch(k16_ctx* ctx, k16_ctx::Lane& L, hipStream_t st, const SortArgs& a, Tick&& tick)
{
    int            rc;
    const void*    d_scalars = a.d_scalars;
    const uint64_t n = a.n;
    const unsigned c = a.c, W = a.W;
    const bool     flat = a.flat;
    const uint32_t nb = a.nb, seg = a.seg, big_cap = a.big_cap;
    const size_t   max_segs = a.max_segs, zr_words = a.zr_words;
    uint32_t *zr = a.zr, *misc = a.misc, *gcount = a.gcount, *gcursor = a.gcursor, *seg_hist = a.seg_hist, *counts = a.counts,
             *offsets = a.offsets, *cursor = a.cursor, *seg_off = a.seg_off, *sorted = a.sorted, *scan_tmp = a.scan_tmp,
             *big_list = a.big_list, *seg_bucket = a.seg_bucket, *seg_order = a.seg_order;
    const void* conv_in  = a.conv_in;
    void*       conv_out = a.conv_out;
    const uint32_t* remap = a.remap;
    // A zero-row mask is an optimisation -- a (0,0) row adds nothing (curve.cpp:185-250) -- and only the partition sort
    // implements it: the generic sort (n > 2^24, K16_ATOMIC_SORT) sorts ALL rows instead of refusing the MSM (round 4 returned
    // K16_ERR_ARG here, which failed every proof of a key with more than 2^24 wires, ADVICE r4).  The lane still records the
    // mask it was ASKED for, so that a later MSM with the same mask reuses the (superset) sort.
    const bool      use_part = flat || (n <= (1u << 24) && !ctx->tune.atomic_sort);
    const uint64_t* skip     = use_part ? a.skip : nullptr;
    constexpr size_t GS  = SORT_GS;
    {
        k16_stat_scope ss(ctx, "msm_sort", st);
        tick("pre");
        K16_HIP(ctx, hipMemsetAsync(zr, 0, zr_words * 4, st));
        tick("memset");
        // five-byte entries + LDS-staged scatter (k_part_stage): the H MSM's sort (flat, c = 20) and the 2^20 x c16 MSM
        const bool staged = use_part && !skip && n >= (1u << 16) && ((flat && c == 20) || (!flat && c == 16 && n < (1u << 24)));
        // the scalars of the prover's H MSM: formed by the staged fixed-base sort's counting pass (below), by a kernel of their
        // own in front of every other sort
        const bool hs_fused = a.hs[0] && staged && flat && !a.conv_in;
        if (a.hs[0] && !hs_fused)
            hipLaunchKernelGGL(k_hs_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (uint4*)const_cast<void*>(d_scalars), n,
                               (const k16::Fr*)a.hs[0], (const k16::Fr*)a.hs[1], (const k16::Fr*)a.hs[2]);
        constexpr unsigned SCAN_BLK = SCAN_T * SCAN_PER_DEFAULT;
        const unsigned nblk = (nb + SCAN_BLK - 1) / SCAN_BLK;
        if (nblk > 4096) { // ws_scan holds 2 x 4096 block totals
            ctx->err = "msm: too many buckets for the scan workspace";
            return K16_ERR_ARG;
        }
        const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, 256 * 8);
        auto scans = [&]() {
            hipLaunchKernelGGL(k_scan2_totals<SCAN_PER_DEFAULT>, dim3(nblk), dim3(SCAN_T), 0, st, counts, nb, seg, scan_tmp);
            hipLaunchKernelGGL(k_scan2_apply<SCAN_PER_DEFAULT>, dim3(nblk), dim3(SCAN_T), 0, st, counts, nb, seg, scan_tmp, offsets, cursor,
                               seg_off, misc, big_list, big_cap, big_list + big_cap, big_list + big_cap + GIANT_CAP, seg_bucket,
                               seg_hist);
        };
        if (use_part) {
            // bin starts and slice table, then the partition itself
            if ((rc = k16_ws_reserve(ctx, L.ws_lvl_d, 2 * GS * 4 + (size_t)n * W * 5 + 64))) return rc;
            uint32_t* gstart = (uint32_t*)L.ws_lvl_d.p;
            uint32_t* gslice = gstart + GS;
            uint32_t* part   = gstart + 2 * GS;
            // Plain partition: counting pass, scatter pass (which scans the bin counts itself and whose workgroup 0 writes the
            // bin starts and the slice table), bucket counts, scans, final scatter.  Count + scatter beats one fused pass: the
            // counting pass is a pure streaming read that leaves the entries in L2 for the scatter pass, and a fused workgroup
            // serialises histogram -> scan -> rank (DESIGN_HISTORY.md).
#define K16_PART(CC) K16_PART_CFG(CC, PartCfg<CC>)
#define K16_PART_CFG(CC, CFG)                                                                                     \
    case CC: {                                                                                                   \
        const unsigned nb1   = CFG::NB1;                                                                         \
        const unsigned ntiles = (unsigned)((n + CFG::TILE - 1) / CFG::TILE);                                     \
        const unsigned pgrid  = std::min<unsigned>(ntiles, 256 * 4);                                             \
        const unsigned sgrid = nb1 + (unsigned)(((uint64_t)n * W) / PART_SLICE) + 1;                              \
        static_assert(CFG::NB1 + 1 <= GS, "partition tables too small");                                         \
        if (conv_in)                                                                                             \
            hipLaunchKernelGGL((k_part<CFG, false, true>), dim3(pgrid), dim3(256), ((nb1 + 1) / 2 + nb1) * 4, st,     \
                               (const uint4*)d_scalars, n, gcount, part, (const k16::Aff<k16::Fq>*)conv_in,            \
                               (k16::Aff<k16::Fq>*)conv_out, (const uint32_t*)nullptr, (uint32_t*)nullptr,             \
                               (uint32_t*)nullptr, skip);                                                                  \
        else                                                                                                     \
            hipLaunchKernelGGL((k_part<CFG, false, false>), dim3(pgrid), dim3(256), ((nb1 + 1) / 2 + nb1) * 4, st,    \
                               (const uint4*)d_scalars, n, gcount, part, (const k16::Aff<k16::Fq>*)nullptr,            \
                               (k16::Aff<k16::Fq>*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,              \
                               (uint32_t*)nullptr, skip);                                                                  \
        hipLaunchKernelGGL((k_part<CFG, true>), dim3(ntiles), dim3(256), ((nb1 + 1) / 2 + nb1) * 4, st, (const uint4*)d_scalars, n, \
                           gcursor, part, (const k16::Aff<k16::Fq>*)nullptr, (k16::Aff<k16::Fq>*)nullptr,         \
                           (const uint32_t*)gcount, gstart, gslice, skip);                                              \
        hipLaunchKernelGGL((k_part_bins<CFG, 0>), dim3(sgrid), dim3(256), 0, st, gstart, gslice, nb1, part, counts, sorted, remap); \
        scans();                                                                                                 \
        hipLaunchKernelGGL((k_part_bins<CFG, 1>), dim3(sgrid), dim3(256), 0, st, gstart, gslice, nb1, part, cursor, sorted, remap); \
    } break;
#define K16_PART_STAGED(CFG)                                                                                      \
    {                                                                                                            \
        const unsigned nb1    = CFG::NB1;                                                                        \
        const unsigned ntiles = (unsigned)((n + CFG::TILE - 1) / CFG::TILE);                                     \
        const unsigned pgrid  = std::min<unsigned>(ntiles, 256 * 4);                                             \
        const unsigned sgrid  = nb1 + (unsigned)(((uint64_t)n * W) / PART_SLICE) + 1;                            \
        const unsigned stiles = (unsigned)((n + CFG::ST_TILE - 1) / CFG::ST_TILE);                               \
        const unsigned slds   = StageGeom<CFG>::LDS_BYTES;                                                       \
        static_assert(CFG::NB1 + 1 <= GS, "partition tables too small");                                         \
        static_assert(StageGeom<CFG>::LDS_BYTES <= 160 * 1024, "stage does not fit the LDS");                    \
        static bool st_attr = false;                                                                             \
        if (!st_attr) {                                                                                          \
            K16_HIP(ctx, hipFuncSetAttribute((const void*)k_part_stage<CFG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)slds)); \
            st_attr = true;                                                                                      \
        }                                                                                                        \
        uint8_t* part1 = (uint8_t*)(part + (size_t)n * W);                                                       \
        if (hs_fused)                                                                                            \
            hipLaunchKernelGGL((k_part<CFG, false, false, true>), dim3(pgrid), dim3(256), ((nb1 + 1) / 2 + nb1) * 4, st, \
                               (const uint4*)d_scalars, n, gcount, part, (const k16::Aff<k16::Fq>*)nullptr,       \
                               (k16::Aff<k16::Fq>*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, \
                               (const uint64_t*)nullptr, (const k16::Fr*)a.hs[0], (const k16::Fr*)a.hs[1],       \
                               (const k16::Fr*)a.hs[2]);                                                         \
        else if (conv_in)                                                                                        \
            hipLaunchKernelGGL((k_part<CFG, false, true>), dim3(pgrid), dim3(256), ((nb1 + 1) / 2 + nb1) * 4, st, \
                               (const uint4*)d_scalars, n, gcount, part, (const k16::Aff<k16::Fq>*)conv_in,       \
                               (k16::Aff<k16::Fq>*)conv_out, (const uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr); \
        else                                                                                                     \
        hipLaunchKernelGGL((k_part<CFG, false, false>), dim3(pgrid), dim3(256), ((nb1 + 1) / 2 + nb1) * 4, st,   \
                           (const uint4*)d_scalars, n, gcount, part, (const k16::Aff<k16::Fq>*)nullptr,           \
                           (k16::Aff<k16::Fq>*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr); \
        hipLaunchKernelGGL(k_bin_starts, dim3(1), dim3(WC_THREADS), 0, st, (const uint32_t*)gcount, nb1, gstart, gslice); \
        hipLaunchKernelGGL((k_part_stage<CFG>), dim3(stiles), dim3(ST_THREADS), slds, st, (const uint4*)d_scalars, n, gcursor, \
                           part, part1, (const uint32_t*)gstart);                                                \
        static bool bs_attr = false;                                                                             \
        const unsigned blds = ((1u << CFG::LO) + BS_THREADS + BS_CAP) * 4;                                       \
        if (!bs_attr) {                                                                                          \
            K16_HIP(ctx, hipFuncSetAttribute((const void*)k_bins_stage<CFG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)blds)); \
            bs_attr = true;                                                                                      \
        }                                                                                                        \
        hipLaunchKernelGGL((k_bins_stage<CFG>), dim3(nb1), dim3(BS_THREADS), blds, st, (const uint32_t*)gstart, nb1,         \
                           (const uint32_t*)part, (const uint8_t*)part1, counts, sorted, remap);                 \
        hipLaunchKernelGGL((k_part_bins<CFG, 0>), dim3(sgrid), dim3(256), 0, st, gstart, gslice, nb1, part, counts, sorted,     \
                           remap, (const uint8_t*)part1, BS_CAP);                                                \
        scans();                                                                                                 \
        hipLaunchKernelGGL((k_part_bins<CFG, 1>), dim3(sgrid), dim3(256), 0, st, gstart, gslice, nb1, part, cursor, sorted,     \
                           remap, (const uint8_t*)part1, BS_CAP);                                                \
    }
            if (staged && flat) {
                K16_PART_STAGED(PartCfgFlat5<20>)
            } else if (staged) {
                K16_PART_STAGED(PartCfg5<16>)
            } else if (flat) {
                switch (c) {
                    K16_PART_CFG(12, PartCfgFlat<12>) K16_PART_CFG(14, PartCfgFlat<14>) K16_PART_CFG(16, PartCfgFlat<16>)
                    K16_PART_CFG(18, PartCfgFlat<18>) K16_PART_CFG(20, PartCfgFlat<20>)
                default: ctx->err = "unsupported fixed-base window size"; return K16_ERR_ARG;
                }
            } else {
                switch (c) {
                    K16_PART(4) K16_PART(5) K16_PART(6) K16_PART(7) K16_PART(8) K16_PART(9) K16_PART(10) K16_PART(11)
                    K16_PART(12) K16_PART(13) K16_PART(14) K16_PART(15) K16_PART(16)
                default: ctx->err = "unsupported window size"; return K16_ERR_ARG;
                }
            }
        } else {
#define K16_DIGITS(CC, SC, ARG0, ARG1)                                                                    \
    case CC: hipLaunchKernelGGL((k_digits<CC, SC>), dim3(grid), dim3(256), 0, st, (const uint4*)d_scalars, n, ARG0, ARG1, remap); break;
#define K16_DIGITS_ALL(SC, ARG0, ARG1)                                                                     \
    switch (c) {                                                                                           \
        K16_DIGITS(4, SC, ARG0, ARG1) K16_DIGITS(5, SC, ARG0, ARG1) K16_DIGITS(6, SC, ARG0, ARG1)          \
        K16_DIGITS(7, SC, ARG0, ARG1) K16_DIGITS(8, SC, ARG0, ARG1) K16_DIGITS(9, SC, ARG0, ARG1)          \
        K16_DIGITS(10, SC, ARG0, ARG1) K16_DIGITS(11, SC, ARG0, ARG1) K16_DIGITS(12, SC, ARG0, ARG1)       \
        K16_DIGITS(13, SC, ARG0, ARG1) K16_DIGITS(14, SC, ARG0, ARG1) K16_DIGITS(15, SC, ARG0, ARG1)       \
        K16_DIGITS(16, SC, ARG0, ARG1)                                                                     \
    default: ctx->err = "unsupported window size"; return K16_ERR_ARG;                                     \
    }
        K16_DIGITS_ALL(false, counts, (uint32_t*)nullptr)
        scans(); // bucket offsets (+ copy into cursor for the scatter), segment offsets, fold classes
        K16_DIGITS_ALL(true, cursor, sorted)
        }
        tick("part+scan");
        // order segments by decreasing length
        const unsigned sgrid = (unsigned)std::min<size_t>((max_segs + 256 * SEG_PER_THREAD - 1) / (256 * SEG_PER_THREAD), 1024);
        hipLaunchKernelGGL(k_seg_scatter, dim3(sgrid), dim3(256), 0, st, offsets, seg_off, misc + 1, seg_bucket, seg_hist,
                           seg_hist + (MAX_SEG + 1), seg_order, seg);
        K16_HIP(ctx, hipGetLastError());
        return K16_OK;
    }
}

// Geometry and workspace of one bucket sort: window count, bucket count, segment length, and the arrays of the sort's
// owner lane SL (reserved unless the sort is being reused).
int msm_sort_plan(k16_ctx* ctx, k16_ctx::Lane& SL, const void* d_scalars, uint64_t n, unsigned c, bool flat, bool reuse,
                  const void* conv_in, void* conv_out, SortArgs* out)
{
    int            rc;
    const unsigned W  = flat ? (257 + c - 1) / c : n_windows(c);
    const uint32_t nb = flat ? (1u << (c - 1)) : (W << (c - 1)); // buckets (w, magnitude - 1) or magnitude - 1
    // Zeroed region of a sort (ONE memset): misc[16] | bin counts[GS] | bin cursors[GS] | segment-length histogram and
    // cursors [2 x (MAX_SEG+1)] | bucket counts[nb+1]
    constexpr size_t GS     = SORT_GS;
    constexpr size_t ZR_HDR = (16 + 2 * GS + 2 * (MAX_SEG + 1) + 3) & ~(size_t)3;
    const size_t     zr_words = ZR_HDR + nb + 1;
    if (!reuse) {
        if ((rc = k16_ws_reserve(ctx, SL.ws_counts, zr_words * 4))) return rc;
        if ((rc = k16_ws_reserve(ctx, SL.ws_offsets, (size_t)(nb + 1) * 4))) return rc;
        if ((rc = k16_ws_reserve(ctx, SL.ws_cursor, (size_t)(nb + 1) * 4))) return rc;
        if ((rc = k16_ws_reserve(ctx, SL.ws_segoff, (size_t)(nb + 1) * 4))) return rc;
        if ((rc = k16_ws_reserve(ctx, SL.ws_sorted, (size_t)n * W * 4))) return rc;
        if ((rc = k16_ws_reserve(ctx, SL.ws_scan, (size_t)(2 * 4096 + 16) * 4))) return rc;
    }
    const uint32_t big_cap = nb; // medium list capacity (every bucket can own many segments when n >> 2^c)
    if (!reuse && (rc = k16_ws_reserve(ctx, SL.ws_big, ((size_t)2 * big_cap + GIANT_CAP) * 4))) return rc;
    // segments: every non-empty bucket has >= 1, plus one per SEG entries
    // segment length: twice the mean bucket load (so an ordinary bucket is one segment), at least MIN_SEG
    uint32_t seg = MIN_SEG;
    // very large uniform MSMs (n >= 2^23 at c = 16: >= 128 entries per bucket): 32-entry segments would leave 4+ partials
    // per bucket to write, read back and fold (2^24 points: 42 ms with 32, 28 ms with 128).  Below that size the short
    // segments stay: they are what keeps skewed (witness) inputs parallel.
    // With signed digits merged into the buckets a uniform MSM loads a bucket with n*W/nb entries on average (32 at
    // n = 2^20, c = 16).  Measured at 2^20 (accumulate + fold): 32 -> 1.31 ms, 48 -> 1.24 ms, 64 -> 1.30 ms: 48 keeps most
    // buckets in one segment without stretching the chains (fewer free first additions, coarser scheduling).
    // General rule: 1.5 x the mean load (a Poisson bucket rarely exceeds it), between 32 and 256.
    {
        const uint64_t mean = (uint64_t)n * W / nb;
        // twice the mean bucket size (1.5x until round 3): with Poisson-sized buckets practically every bucket is then ONE
        // segment, and the fold has next to nothing to do (0.05 -> 0.02 ms at 2^20, +1.5-2 % points/s over 1.5x in two A/B runs of
        // three repetitions; 2.5x, 3x and 4x measure the same: profiles/r03/ab_segment_length.log)
        if (mean >= 24) seg = (uint32_t)std::min<uint64_t>(256, (mean * 2 + 7) & ~7ull);
    }
    if (ctx->forced_seg) seg = ctx->forced_seg; // the prover's witness MSMs: skewed scalars, the mean says nothing
    if (ctx->tune.seg) seg = std::max(1, std::min((int)MAX_SEG, ctx->tune.seg));
    const size_t max_segs = (size_t)nb + (size_t)n * W / seg + 1;
    if (!reuse && (rc = k16_ws_reserve(ctx, SL.ws_segbucket, max_segs * 8 + 64))) return rc;

    uint32_t* zr = (uint32_t*)SL.ws_counts.p;
    SortArgs  a;
    a.d_scalars = d_scalars;
    a.n = n; a.c = c; a.W = W; a.flat = flat; a.nb = nb; a.seg = seg; a.big_cap = big_cap;
    a.max_segs = max_segs; a.zr_words = zr_words;
    a.zr         = zr;
    a.misc       = zr;                 // [0] total entries, [1] total segs, [2] medium, [3] giant, [4] tree count
    a.gcount     = zr + 16;
    a.gcursor    = zr + 16 + GS;
    a.seg_hist   = zr + 16 + 2 * GS;  // [MAX_SEG+1] histogram of segment lengths, then [MAX_SEG+1] cursors
    a.counts     = zr + ZR_HDR;
    a.offsets    = (uint32_t*)SL.ws_offsets.p;
    a.cursor     = (uint32_t*)SL.ws_cursor.p;
    a.seg_off    = (uint32_t*)SL.ws_segoff.p;
    a.sorted     = (uint32_t*)SL.ws_sorted.p;
    a.scan_tmp   = (uint32_t*)SL.ws_scan.p;
    a.big_list   = (uint32_t*)SL.ws_big.p;   // medium list [big_cap] | giant list [GIANT_CAP] | tree list [big_cap]
    a.seg_bucket = (uint32_t*)SL.ws_segbucket.p;
    a.seg_order  = a.seg_bucket + max_segs;
    a.conv_in    = conv_in;
    a.conv_out   = conv_out;
    a.remap      = nullptr;
    a.skip       = nullptr;
    a.hs[0] = a.hs[1] = a.hs[2] = nullptr;
    *out         = a;
    return K16_OK;
}

// Does msm_sort_launch take the plain two-level partition (k_part count + scatter, four-byte entries in the owner lane's
// ws_lvl_d) for this MSM?  Only such a partition can be read again by msm_sort_derive_launch.
static bool msm_sort_is_plain_partition(const k16_ctx* ctx, uint64_t n, unsigned c, bool flat, const uint64_t* skip)
{
    if (flat || n > (1u << 24) || c < 4 || c > 16 || ctx->tune.atomic_sort) return false;
    const bool staged = !skip && n >= (1u << 16) && c == 16 && n < (1u << 24);
    return !staged;
}

// A second set of bucket lists from the PARTITION of another lane's sort (same scalars, same window size), without the
// points whose bit is set in `drop`: pass 3 (bucket counts, scans, final scatter) and the segment order again, into this
// lane's own arrays (a); the scalars are not read, nothing is partitioned.  For a table that shares its scalars with the
// owner's table but has many (0,0) rows of its own (B1 / B2 of a Groth16 key beside A): its accumulation then walks
// segments that hold live rows only.
int msm_sort_derive_launch(k16_ctx* ctx, hipStream_t st, const SortArgs& a, const k16_ctx::Lane& owner, const uint64_t* drop)
{
    const uint32_t*  gstart = (const uint32_t*)owner.ws_lvl_d.p;
    const uint32_t*  gslice = gstart + SORT_GS;
    const uint32_t*  part   = gstart + 2 * SORT_GS;
    k16_stat_scope   ss(ctx, "msm_sort", st);
    K16_HIP(ctx, hipMemsetAsync(a.zr, 0, a.zr_words * 4, st));
    constexpr unsigned SCAN_BLK = SCAN_T * SCAN_PER_DEFAULT;
    const unsigned     nblk     = (a.nb + SCAN_BLK - 1) / SCAN_BLK;
    if (nblk > 4096) {
        ctx->err = "msm: too many buckets for the scan workspace";
        return K16_ERR_ARG;
    }
    const unsigned sgrid_max = (unsigned)(((uint64_t)a.n * a.W) / PART_SLICE) + 1;
#define K16_DERIVE(CC)                                                                                                       \
    case CC: {                                                                                                               \
        typedef PartCfg<CC> CFG;                                                                                             \
        const unsigned      nb1 = CFG::NB1, sgrid = nb1 + sgrid_max;                                                         \
        hipLaunchKernelGGL((k_part_bins<CFG, 0>), dim3(sgrid), dim3(256), 0, st, gstart, gslice, nb1, part, a.counts, a.sorted, \
                           a.remap, (const uint8_t*)nullptr, 0u, drop);                                                      \
        hipLaunchKernelGGL(k_scan2_totals<SCAN_PER_DEFAULT>, dim3(nblk), dim3(SCAN_T), 0, st, a.counts, a.nb, a.seg, a.scan_tmp); \
        hipLaunchKernelGGL(k_scan2_apply<SCAN_PER_DEFAULT>, dim3(nblk), dim3(SCAN_T), 0, st, a.counts, a.nb, a.seg, a.scan_tmp, \
                           a.offsets, a.cursor, a.seg_off, a.misc, a.big_list, a.big_cap, a.big_list + a.big_cap,            \
                           a.big_list + a.big_cap + GIANT_CAP, a.seg_bucket, a.seg_hist);                                    \
        hipLaunchKernelGGL((k_part_bins<CFG, 1>), dim3(sgrid), dim3(256), 0, st, gstart, gslice, nb1, part, a.cursor, a.sorted, \
                           a.remap, (const uint8_t*)nullptr, 0u, drop);                                                      \
    } break;
    switch (a.c) {
        K16_DERIVE(4) K16_DERIVE(5) K16_DERIVE(6) K16_DERIVE(7) K16_DERIVE(8) K16_DERIVE(9) K16_DERIVE(10) K16_DERIVE(11)
        K16_DERIVE(12) K16_DERIVE(13) K16_DERIVE(14) K16_DERIVE(15) K16_DERIVE(16)
    default: ctx->err = "unsupported window size"; return K16_ERR_ARG;
    }
#undef K16_DERIVE
    const unsigned segrid = (unsigned)std::min<size_t>((a.max_segs + 256 * SEG_PER_THREAD - 1) / (256 * SEG_PER_THREAD), 1024);
    hipLaunchKernelGGL(k_seg_scatter, dim3(segrid), dim3(256), 0, st, a.offsets, a.seg_off, a.misc + 1, a.seg_bucket, a.seg_hist,
                       a.seg_hist + (MAX_SEG + 1), a.seg_order, a.seg);
    K16_HIP(ctx, hipGetLastError());
    return K16_OK;
}

template <class E>
int msm_enqueue_t(k16_ctx* ctx, const typename E::Row* d_bases, const void* d_scalars, uint64_t n, unsigned c,
                  bool flat = false, const void* conv_in = nullptr)
{
    // conv_in: a reference-format G1 table still to be converted into d_bases (see k_part); only with the LDS partition
    // sort, which the caller has checked (msm_fuse_convert_ok)
    void* conv_out = conv_in ? (void*)d_bases : nullptr;
    // flat: d_bases is a fixed-base window table (row w*n + i = 2^(c*w) * P_i), all digit positions share one bucket set
    const unsigned W  = flat ? (257 + c - 1) / c : n_windows(c);
    const uint32_t nb = flat ? (1u << (c - 1)) : (W << (c - 1)); // buckets (w, magnitude - 1) or magnitude - 1
    if (flat && (uint64_t)n * W >= (1ull << 25)) {
        ctx->err = "fixed-base msm: n * windows must stay below 2^25";
        return K16_ERR_ARG;
    }
    k16_ctx::Lane& L  = ctx->lanes[ctx->cur_lane];
    hipStream_t    st = k16_lane_stream(ctx, ctx->cur_lane);

    // SL: the lane that owns the bucket sort this MSM reads (its own, unless the caller asked to reuse another lane's)
    int src_lane = (ctx->reuse_sort && ctx->reuse_sort_lane >= 0 && ctx->reuse_sort_lane < k16_ctx::N_LANES)
                       ? ctx->reuse_sort_lane : ctx->cur_lane;
    const uint64_t* acc_skip = ctx->acc_skip_next; // this TABLE's (0,0) rows, stepped over by its accumulation (k_accumulate_skip)
    ctx->acc_skip_next       = nullptr;
    const uint64_t* skip = ctx->skip_next; // (0,0) rows of the table(s) this sort serves, left out of it (k16_msm_set_zero_row_mask)
    ctx->skip_next       = nullptr;
    // derive_lane: bucket lists of this lane's own from that lane's PARTITION, without the rows in `skip`
    // (msm_sort_derive_launch).  Where that lane's sort took another route, its lists are read as they are and the
    // accumulation steps over the rows instead.
    const int derive_lane = ctx->derive_lane;
    ctx->derive_lane      = -1;
    bool derive = false, derive_fallback = false;
    if (derive_lane >= 0) {
        if (derive_lane >= k16_ctx::N_LANES || derive_lane == ctx->cur_lane || !skip || ctx->reuse_sort) {
            ctx->err = "msm: a derived bucket sort needs another lane's sort, a row mask, and no reuse request";
            return K16_ERR_ARG;
        }
        const k16_ctx::Lane& D = ctx->lanes[derive_lane];
        if (!(D.sorted_scalars == d_scalars && D.sorted_n == n && D.sorted_c == c)) {
            ctx->err = "msm: no matching bucket sort on the lane to derive from";
            return K16_ERR_ARG;
        }
        if (D.sorted_plain_partition && !flat) {
            derive = true;
        } else {
            derive_fallback = true;
            src_lane        = derive_lane;
            if (!acc_skip) acc_skip = skip;
        }
    }
    k16_ctx::Lane& SL  = ctx->lanes[src_lane];
    // Measurement probes (results are WRONG or stale on purpose): what would a step cost if the bucket sort / the fold +
    // weighted sum were free?  They exist only in a LAB build of the library (build_alt.sh NAME -DK16_LAB; the variable is
    // K16_LAB_PROBE=nosort / notail / nosort,notail, bench.py with K16_BENCH_NOCHECK=1): libk16.so contains neither the code
    // nor the name, so an inherited environment variable cannot make a production process return stale sums.
#ifdef K16_LAB
    static const char* probe        = getenv("K16_LAB_PROBE");
    static const bool  probe_nosort = probe && strstr(probe, "nosort"), probe_notail = probe && strstr(probe, "notail");
    if (probe_nosort && L.sorted_scalars == d_scalars) ctx->reuse_sort = true;
#else
    constexpr bool probe_notail = false;
#endif
    const bool reuse   = derive_fallback || (ctx->reuse_sort && SL.sorted_scalars == d_scalars && SL.sorted_n == n &&
                                             SL.sorted_c == c && SL.sorted_skip == skip);
    ctx->reuse_sort      = false;
    ctx->reuse_sort_lane = -1;
    if (!reuse && &SL != &L) {
        ctx->err = "msm: no matching bucket sort on the lane to reuse";
        return K16_ERR_ARG;
    }

    int      rc;
    SortArgs sa;
    if ((rc = msm_sort_plan(ctx, SL, d_scalars, n, c, flat, reuse, conv_in, conv_out, &sa))) return rc;
    sa.remap        = ctx->remap_next;
    ctx->remap_next = nullptr;
    sa.skip         = skip;
    for (int k = 0; k < 3; k++) {
        sa.hs[k]        = ctx->hs_next[k];
        ctx->hs_next[k] = nullptr;
    }
    if (sa.hs[0] && (reuse || derive || !sa.hs[1] || !sa.hs[2])) {
        ctx->err = "msm: scalars still to be formed need a bucket sort of their own";
        return K16_ERR_ARG;
    }
    if (sa.remap && flat) {
        ctx->err = "msm: a fixed-base table cannot be combined with a row indirection";
        return K16_ERR_ARG;
    }
    const uint32_t seg = sa.seg, big_cap = sa.big_cap;
    const size_t   max_segs = sa.max_segs;
    uint32_t *misc = sa.misc, *offsets = sa.offsets, *seg_off = sa.seg_off, *sorted = sa.sorted, *big_list = sa.big_list,
             *seg_bucket = sa.seg_bucket, *seg_order = sa.seg_order;
    if ((rc = k16_ws_reserve(ctx, L.ws_lvl_c, (size_t)GIANT_CAP * GIANT_BLOCKS * sizeof(typename E::Pt)))) return rc;
    if ((rc = k16_ws_reserve(ctx, L.ws_partial, max_segs * sizeof(typename E::Pt)))) return rc;
    typename E::Pt*  partial   = (typename E::Pt*)L.ws_partial.p;

    const bool trace = ctx->tune.trace;
#define K16_TRACE_PT(msg)                                                             \
    if (trace) {                                                                      \
        hipError_t te_ = hipStreamSynchronize(st);                                    \
        fprintf(stderr, "[k16 trace] %s : %s\n", msg, hipGetErrorString(te_));       \
    }
    K16_TRACE_PT("enter");
    const bool tick_on = ctx->tune.trace_enq;
    struct Ticks {
        bool on;
        std::chrono::steady_clock::time_point t0, last;
        char buf[512];
        int  len = 0;
        void tick(const char* what)
        {
            if (!on) return;
            auto now = std::chrono::steady_clock::now();
            double ms = std::chrono::duration<double, std::milli>(now - last).count();
            last = now;
            if (ms > 0.3 && len < 440) len += snprintf(buf + len, sizeof buf - len, " %s=%.2f", what, ms);
        }
        ~Ticks()
        {
            if (on && len) fprintf(stderr, "[k16 enq]%s\n", buf);
        }
    } tk{tick_on, std::chrono::steady_clock::now(), std::chrono::steady_clock::now(), {0}};
    if (reuse && &SL != &L) K16_HIP(ctx, hipStreamWaitEvent(st, SL.sort_done, 0));
    const bool use_graphs = ctx->graphs_on && !trace;
    // A captured sort has its kernels' arguments baked in; the key names the scalar array, n, c, the segment length and the
    // sort's shape, NOT the zero-row mask, the row indirection or the drop mask of a derived sort.  Sorts that carry one of
    // those are launched eagerly (ADVICE r4: the same scalars enqueued again with another mask replayed the first mask's
    // graph -- rows silently dropped or kept).
    const bool sort_graphs = use_graphs && !sa.skip && !sa.remap && !skip && !derive;
    // The sort of one MSM: 1 memset + 7 launches (was 4 memsets + 17 launches): counting pass, scatter pass (which scans
    // the bin counts itself), bucket counts, both offset scans + segment map + fold classes in two launches, final
    // scatter, segment order.
    auto sort_body = [&]() -> int { return msm_sort_launch(ctx, L, st, sa, [&](const char* w) { tk.tick(w); }); };
    if (derive) {
        const k16_ctx::Lane& D = ctx->lanes[derive_lane];
        K16_HIP(ctx, hipStreamWaitEvent(st, D.sort_done, 0));
        auto derive_body = [&]() -> int { return msm_sort_derive_launch(ctx, st, sa, D, skip); };
        const k16_ctx::Lane::GraphKey key{-1 - derive_lane, d_scalars, n, c, seg, 0u, 0};
        rc = sort_graphs ? run_graph_section(ctx, L, st, key, derive_body) : derive_body();
        if (rc) return rc;
        L.sorted_scalars         = d_scalars;
        L.sorted_n               = n;
        L.sorted_c               = c;
        L.sorted_skip            = skip;
        L.sorted_plain_partition = false; // the partition is the other lane's
        K16_HIP(ctx, hipEventRecord(L.sort_done, st));
        K16_HIP(ctx, hipStreamWaitEvent(k16_lane_stream(ctx, derive_lane), L.sort_done, 0)); // its next sort overwrites the partition
    } else if (!reuse) {
        const k16_ctx::Lane::GraphKey key{0, d_scalars, n, c, seg, flat ? 1u : 0u, sa.hs[0] ? 1 : 0};
        rc = sort_graphs ? run_graph_section(ctx, L, st, key, sort_body) : sort_body();
        if (rc) return rc;
        L.sorted_scalars         = d_scalars;
        L.sorted_n               = n;
        L.sorted_c               = c;
        L.sorted_skip            = skip;
        L.sorted_plain_partition = msm_sort_is_plain_partition(ctx, n, c, flat, skip);
        K16_HIP(ctx, hipEventRecord(L.sort_done, st));
    }
    tk.tick("sorted");
    K16_TRACE_PT("sorted");
    if (ctx->serialize_acc && ctx->last_acc_done && ctx->last_acc_done != L.acc_done)
        K16_HIP(ctx, hipStreamWaitEvent(st, ctx->last_acc_done, 0));
    {
        k16_stat_scope ss(ctx, "msm_accumulate", st);
        const unsigned grid = (unsigned)std::min<size_t>((max_segs + 127) / 128, 256 * 64);
        if (acc_skip)
            hipLaunchKernelGGL((k_accumulate_skip<E>), dim3(grid), dim3(128 * E::ALPP), 0, st, d_bases, sorted, offsets, seg_off,
                               seg_bucket, seg_order, misc + 1, partial, seg, acc_skip);
        else
            hipLaunchKernelGGL((k_accumulate<E>), dim3(grid), dim3(128 * E::ALPP), 0, st, d_bases, sorted, offsets, seg_off,
                               seg_bucket, seg_order, misc + 1, partial, seg);
    }
    if (ctx->serialize_acc) {
        K16_HIP(ctx, hipEventRecord(L.acc_done, st));
        ctx->last_acc_done = L.acc_done;
    }
    tk.tick("acc");
    K16_TRACE_PT("accumulated");
    // weighted-sum geometry (host side; also what k16_msm_finish needs to combine the partial sums)
    // flat: the 2^(c-1) magnitudes are cut into Wr pseudo-windows of <= 2^15 (the per-window kernels stay as they are)
    const uint32_t Wr      = flat ? std::max<uint32_t>(1u, (1u << (c - 1)) >> 15) : W;
    const uint32_t win_mag = flat ? (1u << (c - 1)) / Wr : (1u << (c - 1)); // magnitudes per (pseudo-)window
    // M = 2^mlog slots per lane: as many as the cap allows, but keep at least ~16 k lanes in flight
    uint32_t mlog = std::min<uint32_t>(ctx->wsum_mlog_cap, WSUM_MLOG_MAX);
    while (mlog > 0 && (((uint64_t)Wr * win_mag) >> mlog) < 16384) mlog--;
    const uint32_t U     = win_mag >> mlog; // digit magnitudes 1 .. win_mag, M per lane (c >= 4)
    uint32_t       nbits = 0;
    while ((1u << nbits) < U) nbits++;
    ctx->pend_mlog  = mlog;
    ctx->pend_nbits = nbits;
    ctx->pend_wr    = Wr;
    if ((size_t)Wr * (nbits + 2) * sizeof(typename E::Pt) > k16_ctx::NARROW_OFF) {
        ctx->err = "msm: pinned staging slot too small";
        return K16_ERR_ARG;
    }
    auto tail_body = [&]() -> int {
    if (probe_notail) return K16_OK;
    {
        k16_stat_scope ss(ctx, "msm_fold", st);
        typename E::Pt* giant_scratch = (typename E::Pt*)L.ws_lvl_c.p;
        const uint32_t  nS = std::min<uint32_t>((nb + 255) / 256, 4096), nT = 512, nB = 256;
        hipLaunchKernelGGL((k_fold_all<E>), dim3(nS + nT + nB + GIANT_BLOCKS), dim3(256 * E::LPP), 256 * sizeof(typename E::Pt), st,
                           seg_off, nb, big_list + big_cap + GIANT_CAP, big_list, big_list + big_cap, misc, big_cap, partial,
                           giant_scratch, nS, nT, nB);
        hipLaunchKernelGGL((k_fold_giant_b<E>), dim3(8), dim3(64 * E::LPP), 64 * sizeof(typename E::Pt), st, seg_off,
                           big_list + big_cap, misc + 3, partial, giant_scratch);
    }
    tk.tick("fold");
    K16_TRACE_PT("folded");
    {
        k16_stat_scope ss(ctx, "msm_reduce", st);
        size_t lb = (size_t)Wr * U * sizeof(typename E::Pt);
        if ((rc = k16_ws_reserve(ctx, L.ws_lvl_a, lb))) return rc;
        if ((rc = k16_ws_reserve(ctx, L.ws_lvl_b, lb))) return rc;
        typename E::Pt* S = (typename E::Pt*)L.ws_lvl_a.p;
        typename E::Pt* G = (typename E::Pt*)L.ws_lvl_b.p;
        // the <= 240 partial sums go straight into this MSM's pinned staging slot (device-mapped host memory): no copy
        // command; k16_msm_finish reads them after the event recorded behind this kernel
        typename E::Pt* T = (typename E::Pt*)((char*)ctx->pinned_dev + (size_t)ctx->enq_slot * k16_ctx::SLOT_BYTES);
        unsigned nthr = 2 * Wr * U; // lane pairs
        // the prefetching variant for the single MSM on a proof's critical path (the fixed-base H MSM); the pipelined MSMs and
        // the witness MSMs keep the two-point version (fewer registers beside other lanes' kernels)
        if (flat && sizeof(typename E::Pt) < 200)
            hipLaunchKernelGGL((k_wsum_level1<E, true>), dim3((nthr + 63) / 64), dim3(64 * E::LPP), 0, st, U, Wr, 1u << mlog, seg_off, c,
                               flat ? 1u : 0u, partial, S, G);
        else
            hipLaunchKernelGGL((k_wsum_level1<E>), dim3((nthr + 63) / 64), dim3(64 * E::LPP), 0, st, U, Wr, 1u << mlog, seg_off, c,
                               flat ? 1u : 0u, partial, S, G);
        hipLaunchKernelGGL((k_wsum_bits<E>), dim3(Wr * (nbits + 2)), dim3(256 * E::LPP), 256 * sizeof(typename E::Pt), st, S, G, U, nbits,
                           T);
        tk.tick("wsum");
    }
    tk.tick("d2h");
    K16_TRACE_PT("reduced");
    K16_HIP(ctx, hipGetLastError());
    return K16_OK;
    };
    {
        // the tail's launches depend on the sort owner's arrays too (seg_off ...): the source lane is part of the key
        const k16_ctx::Lane::GraphKey key{1 + (int)sizeof(typename E::Pt), (const void*)&SL, n, c,
                                          seg * 64u + mlog, flat ? 1u : 0u, ctx->enq_slot};
        return use_graphs ? run_graph_section(ctx, L, st, key, tail_body) : tail_body();
    }
}

// ------------------------------------------------------------------------------------------
// Scalar-class MSM (k16_msm_enqueue_classified).  The scalars of a Groth16 witness MSM are ~45 % zeros, ~45 % ones,
// ~8 % bytes and ~2 % field elements; the reference's `if (chunkValue)` (multiexp.cpp:59-65) makes such an MSM cheap on a
// CPU -- a bit-valued wire touches one bucket of one window -- while the bucket pipeline above pays for its skew: one
// bucket with 45 % of the points, tens of thousands of empty buckets in the weighted sum, latency-bound folds.
// Here the scalars below 256 never see a bucket:
//     sum_i s_i P_i  =  sum_{b < 8} 2^b * S_b  +  MSM(wide scalars),      S_b = sum of the P_i with bit b of s_i set
// The lists "wires with bit b set" come from ONE classification of the scalar vector (msm_classes.hip; shared by every
// table that is indexed by the same wires, rows that are (0,0) in a table left out of that table's lists), a masked sum is
// a plain reduction: strided chains of mixed additions per lane, an LDS tree per workgroup, one more tree per list.  The
// few wide scalars (a compacted array + their wire numbers as a row indirection of the sort) take the ordinary path.
// Same group element as the reference's sum; the 2^b and the addition of the two parts are the host's (k16_msm_finish).
// ------------------------------------------------------------------------------------------
constexpr unsigned NARROW_BITS = k16_scalar_classes::BITS;

// lists: the set's BITS lists of capacity cap_n each; cnt: their lengths.  A chunk is 256 * K consecutive entries of one
// list; chunk numbers run list after list.  partial[chunk] = sum of the chunk's rows; chunk_tab[0 .. 8] (written by
// workgroup 0) = first chunk of every list, [8] = number of chunks.
template <class E>
__global__ void __launch_bounds__(256) k_masked_sums(const typename E::Row* __restrict__ bases, const uint32_t* __restrict__ lists,
                                                     uint64_t cap_n, const uint32_t* __restrict__ cnt, uint32_t K,
                                                     typename E::Pt* __restrict__ partial, uint32_t* __restrict__ chunk_tab)
{
    k16_short_kernel_prio();
    extern __shared__ uint4 lds_raw[];
    typename E::Pt*         lds = reinterpret_cast<typename E::Pt*>(lds_raw);
    __shared__ uint32_t     pre[NARROW_BITS + 1], len[NARROW_BITS];
    const uint32_t          CH = 256u * K;
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (unsigned b = 0; b < NARROW_BITS; b++) {
            pre[b] = run;
            len[b] = cnt[b];
            run += (len[b] + CH - 1) / CH;
        }
        pre[NARROW_BITS] = run;
    }
    k16_lds_sync();
    if (blockIdx.x == 0 && threadIdx.x <= NARROW_BITS) chunk_tab[threadIdx.x] = pre[threadIdx.x];
    for (uint32_t chunk = blockIdx.x; chunk < pre[NARROW_BITS]; chunk += gridDim.x) {
        unsigned b = 0;
        while (b + 1 < NARROW_BITS && pre[b + 1] <= chunk) b++;
        const uint32_t* __restrict__ list = lists + (size_t)b * cap_n;
        const uint32_t lo = (chunk - pre[b]) * CH, hi = min(lo + CH, len[b]);
        typename E::Pt acc = E::zero();
        uint32_t       j   = lo + threadIdx.x;
        if (j < hi) {
            typename E::AffR nxt = E::load_row(&bases[list[j]]);
            if constexpr (E::has_aff_add) {
                if (j + 256 < hi) {
                    typename E::AffR first = nxt, second = E::load_row(&bases[list[j + 256]]);
                    if (j + 512 < hi) nxt = E::load_row(&bases[list[j + 512]]);
                    acc = E::add_aff(first, second);
                    j += 512;
                }
            }
#pragma clang loop unroll(disable)
            for (; j < hi; j += 256) {
                typename E::AffR cur = nxt;
                if (j + 256 < hi) nxt = E::load_row(&bases[list[j + 256]]); // the next row flies during this addition
                acc = E::madd(acc, cur);
            }
        }
        lds[threadIdx.x] = acc;
        k16_lds_sync();
#pragma clang loop unroll(disable)
        for (unsigned o = 128; o > 0; o >>= 1) {
            if (threadIdx.x < o) {
                typename E::Pt a = lds[threadIdx.x], c = lds[threadIdx.x + o];
                lds[threadIdx.x] = E::add(a, c);
            }
            k16_lds_sync();
        }
        if (threadIdx.x == 0) store_vec(&partial[chunk], lds[0]);
        k16_lds_sync();
    }
}
// workgroup b: out[b] = sum of list b's chunk sums
template <class E>
__global__ void __launch_bounds__(256) k_masked_final(const typename E::Pt* __restrict__ partial, const uint32_t* __restrict__ chunk_tab,
                                                      typename E::Pt* __restrict__ out)
{
    k16_short_kernel_prio();
    extern __shared__ uint4 lds_raw[];
    typename E::Pt*         lds = reinterpret_cast<typename E::Pt*>(lds_raw);
    const uint32_t          lo = chunk_tab[blockIdx.x], hi = chunk_tab[blockIdx.x + 1];
    typename E::Pt          acc = E::zero();
#pragma clang loop unroll(disable)
    for (uint32_t j = lo + threadIdx.x; j < hi; j += 256) acc = E::add(acc, load_vec(&partial[j]));
    lds[threadIdx.x] = acc;
    k16_lds_sync();
#pragma clang loop unroll(disable)
    for (unsigned o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o && threadIdx.x + o < hi - lo) { // (an empty operand would only cost an addition's early exit)
            typename E::Pt a = lds[threadIdx.x], c = lds[threadIdx.x + o];
            lds[threadIdx.x] = E::add(a, c);
        }
        k16_lds_sync();
    }
    if (threadIdx.x == 0) store_vec(&out[blockIdx.x], lds[0]);
}

// The classified MSM of one table on the current lane: masked sums of the set's lists into the staging slot's narrow
// area, then -- when there are wide scalars -- the ordinary MSM over them (bucket sort shared between the tables through
// reuse_sort as before, its entries mapped to wire numbers).  *has_wide tells the caller whether window sums were staged.
template <class E>
int msm_enqueue_classified_t(k16_ctx* ctx, const typename E::Row* d_rows, const k16_scalar_classes* cls, int set, unsigned c,
                             bool* has_wide, int phase)
{
    int            rc;
    k16_ctx::Lane& L  = ctx->lanes[ctx->cur_lane];
    hipStream_t    st = k16_lane_stream(ctx, ctx->cur_lane);
    K16_HIP(ctx, hipStreamWaitEvent(st, cls->built, 0));
    // entries per lane of a masked sum: a chain of K dependent additions, then the trees.  Longer chains are less work per
    // entry (the trees' 255 full additions per 256 * K mixed ones), shorter ones finish sooner; G2 additions take 3x as long
    const unsigned K = sizeof(typename E::Pt) > 200 ? 16u : 32u; // G2 : G1
    const uint64_t max_chunks = ((uint64_t)NARROW_BITS * cls->n + 256ull * K - 1) / (256ull * K) + NARROW_BITS;
    if ((rc = k16_ws_reserve(ctx, L.ws_narrow, 64 + max_chunks * sizeof(typename E::Pt)))) return rc;
    uint32_t*       chunk_tab = (uint32_t*)L.ws_narrow.p;
    typename E::Pt* partial   = (typename E::Pt*)((char*)L.ws_narrow.p + 64);
    typename E::Pt* out = (typename E::Pt*)((char*)ctx->pinned_dev + (size_t)ctx->enq_slot * k16_ctx::SLOT_BYTES + k16_ctx::NARROW_OFF);
    auto narrow = [&]() -> int {
        k16_stat_scope ss(ctx, "msm_narrow", st);
        const unsigned grid = (unsigned)std::min<uint64_t>(max_chunks, 1024);
        hipLaunchKernelGGL((k_masked_sums<E>), dim3(grid), dim3(256), 256 * sizeof(typename E::Pt), st, d_rows,
                           cls->d_lists + (size_t)set * NARROW_BITS * cls->cap_n, cls->cap_n,
                           cls->d_cnt + set * NARROW_BITS, K, partial, chunk_tab);
        hipLaunchKernelGGL((k_masked_final<E>), dim3(NARROW_BITS), dim3(256), 256 * sizeof(typename E::Pt), st, partial, chunk_tab, out);
        K16_HIP(ctx, hipGetLastError());
        return K16_OK;
    };
    *has_wide = cls->n_wide != 0;
    // phase 1: the masked sums only; phase 2: the wide part only (the prover enqueues the four tables' masked sums first --
    // they then run beside the SpMV, whose lanes wait on gathers, instead of beside the NTT passes -- and the wide parts after)
    if (phase == 1) return narrow();
    if (!*has_wide) {
        ctx->reuse_sort      = false;
        ctx->reuse_sort_lane = -1;
        return phase == 2 ? K16_OK : narrow();
    }
    // the MSM that owns the bucket sort of the wide scalars runs it FIRST: the other tables' MSMs (other lanes) wait for it
    const bool owns_sort = !ctx->reuse_sort;
    if (phase == 0 && !owns_sort && (rc = narrow())) return rc;
    ctx->remap_next = cls->d_wide_idx;
    if ((rc = msm_enqueue_t<E>(ctx, d_rows, cls->d_wide_scalars, cls->n_wide, c))) return rc;
    return (phase == 0 && owns_sort) ? narrow() : K16_OK;
}

} // namespace
