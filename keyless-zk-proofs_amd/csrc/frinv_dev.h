// frinv_dev.h -- the device Fr inversion the set-up (setup.hip), the second-value scan and the witness completion (r1cs_scan.hip) share.
#pragma once
#include "bn254_fq9.h"

namespace k16 {
namespace {

__device__ __forceinline__ Fr9 fr9_one()
{
    Fr9 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = Fr9C::ONE[i];
    return r;
}
// a^(r-2) in the R' domain; a < 2r, a != 0 mod r
__device__ __noinline__ Fr9 frinv9(const Fr9& a)
{
    Fr9 r = fr9_one();
#pragma clang loop unroll(disable)
    for (int bit = 253; bit >= 0; bit--) {
        const uint32_t e = FrParams::P[bit >> 5] - (bit < 32 ? 2u : 0u); // r - 2: the low word is 0xf0000001, no borrow
        r = frmul9(r, r);
        if ((e >> (bit & 31)) & 1u) r = frmul9(r, a);
    }
    return r;
}

} // namespace
} // namespace k16
