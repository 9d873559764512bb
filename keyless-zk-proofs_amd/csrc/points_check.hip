// points_check.hip -- batched validation of encoded points (include/k16.h: k16_points_check; the G2 subgroup part of
// k16_verify_batch_checked and k16_zkey_check): canonical coordinates, on the curve / the twist, and -- for G2 -- membership
// in the order-r subgroup by the endomorphism test of bn254_points.h (eprint 2022/348, section 5.1).
//
// Layout: one lane per G1 point (a few canonical 8 x 32-bit products), one LANE PAIR per G2 point -- the Fq2 arithmetic of
// the ~94-operation chain on bn254_fq2pair.h's Fq2h (each lane one component, radix 2^29), the point and the constants in
// registers, no LDS.  A lone pair is what the checked verifier's small batches run beside the wave-cooperative pairing.
#include <string.h>
#include <algorithm>
#include "points_check.h"
#include "bn254_fq2pair.h"

namespace k16 {
// Fq2h as the F of bn254_points.h's test: conjugation negates the odd lane's component; a canonical constant becomes the
// component this lane holds
__device__ __forceinline__ Fq2h g2_conj(const Fq2h& x) { return pair_is_odd() ? fneg(x) : x; }
__device__ __forceinline__ void fq2_to(const Fq2& x, Fq2h& out) { out.v = fq9_from_fq(pair_is_odd() ? x.b : x.a); }
} // namespace k16

using namespace k16;

namespace {

__device__ __forceinline__ void ld_words(uint32_t* w, const uint8_t* p, int n16)
{
    const uint4* s = reinterpret_cast<const uint4*>(p);
    for (int i = 0; i < n16; i++) {
        const uint4 v = s[i];
        w[4 * i] = v.x, w[4 * i + 1] = v.y, w[4 * i + 2] = v.z, w[4 * i + 3] = v.w;
    }
}
__device__ __forceinline__ G1Aff ld_g1(const uint8_t* p)
{
    G1Aff a;
    uint32_t w[16];
    ld_words(w, p, 4);
#pragma unroll
    for (int k = 0; k < 8; k++) a.x.v[k] = w[k], a.y.v[k] = w[8 + k];
    return a;
}
__device__ __forceinline__ G2Aff ld_g2(const uint8_t* p)
{
    G2Aff b;
    uint32_t w[32];
    ld_words(w, p, 8);
#pragma unroll
    for (int k = 0; k < 8; k++) b.x.a.v[k] = w[k], b.x.b.v[k] = w[8 + k], b.y.a.v[k] = w[16 + k], b.y.b.v[k] = w[24 + k];
    return b;
}

// the lead lane of a point writes its status (if asked) and folds a failure into sum: [0] the smallest key, [1] the count
__device__ __forceinline__ void report(uint64_t i, uint8_t st, bool lead, uint8_t* status, uint64_t* sum, uint64_t key_base)
{
    if (lead && status) status[i] = st;
    const bool     bad  = lead && st != PT_OK;
    const uint64_t mask = __ballot(bad);
    if (!mask) return;
    if (bad) atomicMin((unsigned long long*)sum, (unsigned long long)(key_base + ((i << 2) | st)));
    if ((threadIdx.x & 63) == (unsigned)(__ffsll((unsigned long long)mask) - 1))
        atomicAdd((unsigned long long*)(sum + 1), (unsigned long long)__popcll(mask));
}

__global__ void __launch_bounds__(256) k_points_check_g1(const uint8_t* __restrict__ pts, uint64_t n, uint8_t* __restrict__ status,
                                                         uint64_t* __restrict__ sum, uint64_t key_base)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    report(i, g1_point_status(ld_g1(pts + i * 64)), true, status, sum, key_base);
}

__global__ void __launch_bounds__(256) k_points_check_g2(const uint8_t* __restrict__ pts, uint64_t n, uint8_t* __restrict__ status,
                                                         uint64_t* __restrict__ sum, uint64_t key_base, G2Consts K)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, i = t >> 1;
    if (i >= n) return; // both lanes of the pair
    const uint8_t st = g2_point_status<Fq2h>(ld_g2(pts + i * 128), K);
    report(i, st, (t & 1) == 0, status, sum, key_base);
}

// proof i: A (64 B) | B (128 B) | C (64 B); reason[i] = the first failing point's status
__global__ void __launch_bounds__(256) k_proofs_check(const uint8_t* __restrict__ proofs, uint64_t n, uint8_t* __restrict__ reason,
                                                      G2Consts K)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, i = t >> 1;
    if (i >= n) return;
    const uint8_t* pr = proofs + i * 256;
    uint8_t        st = g1_point_status(ld_g1(pr));
    if (st == PT_OK) st = g2_point_status<Fq2h>(ld_g2(pr + 64), K);
    if (st == PT_OK) st = g1_point_status(ld_g1(pr + 192));
    if ((t & 1) == 0) reason[i] = st;
}

} // namespace

namespace k16 {

int launch_proofs_check(hipStream_t st, const uint8_t* d_proofs, uint64_t n, uint8_t* d_reason)
{
    if (n == 0) return K16_OK;
    hipLaunchKernelGGL(k_proofs_check, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, st, d_proofs, n, d_reason,
                       g2_consts_host());
    return hipGetLastError() == hipSuccess ? K16_OK : K16_ERR_HIP;
}

int PointsStream::begin(k16_ctx* c, size_t max_bytes)
{
    ctx = c;
    cap = (std::min<size_t>(PTS_CHUNK_BYTES, std::max<size_t>(max_bytes, 128)) + 127) & ~(size_t)127; // whole G1 and G2 points
    K16_HIP(ctx, hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
    for (int b = 0; b < 2; b++) {
        K16_HIP(ctx, hipEventCreateWithFlags(&copied[b], hipEventDisableTiming));
        K16_HIP(ctx, hipEventCreateWithFlags(&done[b], hipEventDisableTiming));
        K16_HIP(ctx, hipMalloc((void**)&d_pts[b], cap));
        K16_HIP(ctx, hipHostMalloc((void**)&h_st[b], cap / 64, hipHostMallocMapped | hipHostMallocCoherent));
        K16_HIP(ctx, hipHostGetDevicePointer((void**)&d_st[b], h_st[b], 0));
    }
    K16_HIP(ctx, hipMalloc((void**)&d_sum, 2 * sizeof(uint64_t)));
    K16_HIP(ctx, hipMemsetAsync(d_sum, 0xff, sizeof(uint64_t), ctx->stream));
    K16_HIP(ctx, hipMemsetAsync(d_sum + 1, 0, sizeof(uint64_t), ctx->stream));
    return K16_OK;
}

int PointsStream::drain(int b)
{
    if (!pend[b]) return K16_OK;
    pend[b] = false;
    K16_HIP(ctx, k16_event_wait(ctx, done[b]));
    if (pend_out[b]) memcpy(pend_out[b], h_st[b], pend_n[b]);
    return K16_OK;
}

int PointsStream::feed(int group, const uint8_t* h_pts, uint64_t n, uint8_t* h_status, uint64_t key_base)
{
    const uint64_t psz = group == K16_G2 ? 128 : 64, per = cap / psz;
    for (uint64_t off = 0; off < n; off += per, k++) {
        const uint64_t m = std::min(per, n - off);
        const int      b = (int)(k & 1);
        int            rc = drain(b); // chunk k - 2 used buffer b: its check has finished before the copy overwrites it
        if (rc) return rc;
        {
            k16_stat_scope sc(ctx, "points_check_h2d", copy);
            K16_HIP(ctx, hipMemcpyAsync(d_pts[b], h_pts + off * psz, m * psz, hipMemcpyHostToDevice, copy));
        }
        K16_HIP(ctx, hipEventRecord(copied[b], copy));
        K16_HIP(ctx, hipStreamWaitEvent(ctx->stream, copied[b], 0));
        uint8_t* st = h_status ? d_st[b] : nullptr;
        if (group == K16_G2) {
            k16_stat_scope sc(ctx, "points_check_g2");
            hipLaunchKernelGGL(k_points_check_g2, dim3((unsigned)((2 * m + 255) / 256)), dim3(256), 0, ctx->stream, d_pts[b], m, st,
                               d_sum, key_base + (off << 2), g2_consts_host());
        } else {
            k16_stat_scope sc(ctx, "points_check_g1");
            hipLaunchKernelGGL(k_points_check_g1, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, d_pts[b], m, st,
                               d_sum, key_base + (off << 2));
        }
        K16_HIP(ctx, hipGetLastError());
        K16_HIP(ctx, hipEventRecord(done[b], ctx->stream));
        pend[b]     = true;
        pend_out[b] = h_status ? h_status + off : nullptr;
        pend_n[b]   = m;
    }
    return K16_OK;
}

int PointsStream::finish(uint64_t* first_key, uint64_t* n_bad)
{
    for (int b = 0; b < 2; b++) {
        int rc = drain((int)((k + b) & 1)); // the older chunk first
        if (rc) return rc;
    }
    uint64_t h[2];
    K16_HIP(ctx, hipMemcpyAsync(h, d_sum, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    K16_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *first_key = h[0];
    *n_bad     = h[1];
    return K16_OK;
}

PointsStream::~PointsStream()
{
    if (!ctx) return;
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (copy) (void)hipStreamSynchronize(copy);
    for (int b = 0; b < 2; b++) {
        if (d_pts[b]) (void)hipFree(d_pts[b]);
        if (h_st[b]) (void)hipHostFree(h_st[b]);
        if (copied[b]) (void)hipEventDestroy(copied[b]);
        if (done[b]) (void)hipEventDestroy(done[b]);
    }
    if (d_sum) (void)hipFree(d_sum);
    if (copy) (void)hipStreamDestroy(copy);
}

} // namespace k16

// status per point, affine Montgomery LE (G1 64 B, G2 128 B); all-zero = infinity = K16_PT_OK
extern "C" int k16_points_check(k16_ctx* ctx, int group, const void* h_points, uint64_t n, uint8_t* h_status)
{
    return k16_guard(ctx, [&]() -> int {
    if (!ctx || (group != K16_G1 && group != K16_G2) || (n && (!h_points || !h_status))) return K16_ERR_ARG;
    if (n == 0) return K16_OK;
    K16_HIP(ctx, hipSetDevice(ctx->device));
    PointsStream ps;
    int          rc = ps.begin(ctx, (size_t)n * (group == K16_G2 ? 128 : 64));
    if (!rc) rc = ps.feed(group, (const uint8_t*)h_points, n, h_status, 0);
    uint64_t first = 0, bad = 0;
    if (!rc) rc = ps.finish(&first, &bad);
    return rc;
    });
}
