// spmv_dev.h -- device helpers shared by the prover's k_spmv (prover.hip) and the R1CS witness check's row kernel
// (r1cs_check.hip): 32-byte loads / stores of packed field values and the walk over a plan of spmv_plan.h.
#pragma once
#include <hip/hip_runtime.h>
#include "bn254_field.h"
#include "bn254_fq9.h"
#include "spmv_plan.h"

namespace k16 {

__device__ __forceinline__ Fr ld_fr(const Fr* p)
{
    Fr           r;
    const uint4* s = reinterpret_cast<const uint4*>(p);
    uint4        a = s[0], b = s[1];
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
    r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    return r;
}
__device__ __forceinline__ void st_fr(Fr* p, const Fr& r)
{
    uint4* d = reinterpret_cast<uint4*>(p);
    d[0]     = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
    d[1]     = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
}

// The polynomial chain works on the radix-2^29 representation of Fr (bn254_fq9.h): a, b, c live in HBM as
// packed R' values (x * 2^261 mod r, < 2r, 32 bytes), the coefficients are stored pre-multiplied by 2^522
// (the reference's zkey stores them pre-multiplied by R^2 = 2^512 for the same reason), and only the
// final H scalars are brought back to the canonical standard form the MSM consumes.  Field values are exact
// mod r throughout, so the H scalars are bit-identical to the reference's (tests compare them).
__device__ __forceinline__ Fr9 ld_r9(const Fr* p)
{
    Fr w = ld_fr(p);
    return fr9_load(w.v);
}
__device__ __forceinline__ void st_r9(Fr* p, const Fr9& v)
{
    Fr w;
    fr9_store(w.v, v);
    st_fr(p, w);
}

// entry e of a plan: wtns[wire[e]] * coef9[e] as an R' value.
// n16 (round 4): one 16-bit word per wire -- the value when it is below 256, bit 15 when it is not.  98 % of a circuit's
// wires are bits and bytes: the walk's dependent gather then hits a 2.7 MB array (L2) instead of the 43 MB witness, and
// the product is a single-limb multiplication; only the wide wires load their 32 bytes.  Same integers, same limbs.
__device__ __forceinline__ Fr9 spmv_term(const uint32_t* __restrict__ wire, const Fr* __restrict__ coef9,
                                         const Fr* __restrict__ wtns, const uint16_t* __restrict__ n16, uint32_t e)
{
    const uint32_t wi = wire[e];
    if (n16) {
        const uint32_t c = n16[wi];
        if (!(c & 0x8000u)) return fmul9_small_t<Fr9C>(ld_r9(&coef9[e]), c);
    }
    return frmul9(ld_r9(&wtns[wi]), ld_r9(&coef9[e]));
}

// One wave per slice (64 rows, a lane each, slice.len steps) or per long row (lanes stride over the row's contiguous
// entries, butterfly reduction); store(row, sum) is called once for every row by the lane that owns it.  For kernels
// launched with whole waves, (n_slices + n_long) of them or more.
template <class Store>
__device__ __forceinline__ void spmv_walk(const SpmvSlice* __restrict__ slices, uint32_t n_slices,
                                          const uint32_t* __restrict__ row_of, const SpmvLong* __restrict__ longs,
                                          uint32_t n_long, const uint32_t* __restrict__ wire, const Fr* __restrict__ coef9,
                                          const Fr* __restrict__ wtns, const uint16_t* __restrict__ n16, Store store)
{
    const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    Fr9            acc = fq9_zero();
    if (w < n_slices) {
        const SpmvSlice sl = slices[w];
        for (uint32_t k = 0; k < sl.len; k++) {
            const uint32_t e = sl.off + (k << 6) + lane; // padding entries: wire 0, coefficient 0
            acc = fradd9(acc, spmv_term(wire, coef9, wtns, n16, e));
        }
        const uint32_t row = row_of[(w << 6) + lane];
        if (row != 0xffffffffu) store(row, acc);
        return;
    }
    if (w - n_slices >= n_long) return;
    const SpmvLong L = longs[w - n_slices];
    for (uint32_t k = lane; k < L.len; k += 64) {
        const uint32_t e = L.off + k;
        acc = fradd9(acc, spmv_term(wire, coef9, wtns, n16, e));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        Fr9 o;
#pragma unroll
        for (int i = 0; i < 9; i++) o.l[i] = (uint32_t)__shfl_xor((int)acc.l[i], d, 64);
        acc = fradd9(acc, o);
    }
    if (lane == 0) store(L.row, acc);
}

} // namespace k16
