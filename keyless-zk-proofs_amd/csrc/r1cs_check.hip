// r1cs_check.hip -- the R1CS witness check on the GPU (include/k16.h, k16_r1cs_*): which constraints of a circuit does a
// witness break?  (A.w) o (B.w) - C.w = 0 is three sparse matrix-vector products over Fr and one pointwise pass:
//   k_r1cs_rows    k_spmv's walk (spmv_dev.h) over the 3 M rows A | B | C of the circuit's .r1cs file (r1cs_file.h: length-sorted
//                  slices + a wave per long row), the sum of row id = matrix * M + constraint stored at index id as a packed
//                  R' value -- no bit reversal, no transform follows
//   k_r1cs_judge   one lane per constraint: a * b - c brought to the canonical standard form and compared with zero (the sums
//                  are lazy representatives below 2r: only the canonical form tells r from 0); a wave's verdicts leave as one
//                  64-bit ballot word, written by one lane
// Two kernels because the judge needs all three sums of a constraint and the rows are placed by LENGTH: A_c, B_c and C_c sit in
// different slices, waves and workgroups.  The host reads the mask: an exact count and the failing constraints in ascending
// order, the same for every run (an atomically appended list would come in a different order each time).
// A witness with a wire >= r, or with wire 0 != 1, is refused (K16_ERR_FORMAT) by k_r1cs_wtns, the pass that also makes the
// n16 words of an uploaded witness: every constraint can hold for an assignment with wire 0 = 2, yet no proof of it verifies.
// Under a proof (k16_prover_set_r1cs; ctx.h k16_r1cs_fork / _join) the same three kernels run on a stream the prover names, behind
// the proof's witness upload, and k_r1cs_summary condenses mask and flags into one record in pinned, device-mapped memory: the
// prove call reads 272 bytes at its join instead of copying and walking the mask.
// The unbound-wire scan (k16_r1cs_unbound_wires; r1cs_pairs.h) asks the dual question of the sums a
// completed check left in d_rows: which wires could take any value without moving a residual?
//   k_r1cs_incidences  one lane per (wire, constraint) incidence: is d(a b - c) / d(wire) or the wire's quadratic part non-zero?
//                      A wave ORs the bits of the wires it found bound into a mask of ceil(nWires / 64) words; the host reads it.
// Its list and its buffers are made by the first scan of an object: a circuit that is never scanned pays nothing.
// The second-value scan (k16_r1cs_second_values) walks the same list for the wires that admit exactly
// ONE other value with every other wire held fixed:
//   k_r1cs_kinds   one lane per incidence: PIN (one of lin, quad is zero) or ROOT (neither is)?  Two masks, and per wire the
//                  lowest ROOT incidence -- the wire's reference
//   k_r1cs_agree   one lane per incidence: does a ROOT incidence move the wire by the same d = -lin / quad as the reference does?
//                  Where not, the wire is pinned after all
//   k_r1cs_shifts  one lane per LISTED wire: d from the reference incidence, one inversion, standard form
// The determinism closure (k16_r1cs_determined_wires) asks the global question the two scans leave open:
// given the values of the seed wires (by default the circuit's inputs), which other wires does the circuit force?  A fixed point
// over the same list, a round at a time: k_r1cs_det_init / _first / _derive / _expand, described where they stand.
#include <stdio.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>
#include "ctx.h"
#include "frinv_dev.h"
#include "r1cs_file.h"
#include "r1cs_pairs.h"
#include "spmv_dev.h"

using namespace k16;

static_assert(sizeof(R1csPair) == sizeof(uint4), "an incidence is one 16-byte load");
static_assert(R1CS_ERR_ARG == K16_ERR_ARG && R1CS_ERR_FORMAT == K16_ERR_FORMAT && R1CS_ERR_CURVE == K16_ERR_CURVE && R1CS_OK == K16_OK,
              "r1cs_file.h returns the library's status codes");

namespace {

enum : unsigned long long { WTNS_NOT_BELOW_R = 1, WTNS_WIRE0_NOT_ONE = 2 };

// every wire: below r? wire 0: one?  n16 (may be null: the prover made it already) as k_wtns_n16 of prover.hip makes it
__global__ void __launch_bounds__(256) k_r1cs_wtns(const uint4* __restrict__ wtns, uint32_t n, uint16_t* __restrict__ n16,
                                                   unsigned long long* __restrict__ flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4    lo = wtns[2 * (size_t)i], hi = wtns[2 * (size_t)i + 1];
    const bool     wide = ((lo.x >> 8) | lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w) != 0;
    if (n16) n16[i] = wide ? (uint16_t)0x8000u : (uint16_t)lo.x;
    unsigned long long bad = 0;
    if (hi.w >= FrParams::P[7]) { // (only then can the value reach r)
        const uint32_t v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        bool           geq  = true;
        for (int k = 7; k >= 0; k--) {
            if (v[k] != FrParams::P[k]) {
                geq = v[k] > FrParams::P[k];
                break;
            }
        }
        if (geq) bad |= WTNS_NOT_BELOW_R;
    }
    if (i == 0 && (wide || lo.x != 1u)) bad |= WTNS_WIRE0_NOT_ONE;
    if (bad) atomicOr(flags, bad);
}

__global__ void __launch_bounds__(256) k_r1cs_rows(const SpmvSlice* __restrict__ slices, uint32_t n_slices,
                                                   const uint32_t* __restrict__ row_of, const SpmvLong* __restrict__ longs,
                                                   uint32_t n_long, const uint32_t* __restrict__ wire,
                                                   const Fr* __restrict__ coef9, const Fr* __restrict__ wtns,
                                                   const uint16_t* __restrict__ n16, Fr* __restrict__ rows)
{
    spmv_walk(slices, n_slices, row_of, longs, n_long, wire, coef9, wtns, n16,
              [&](uint32_t row, const Fr9& acc) { st_r9(&rows[row], acc); });
}

// rows: A.w | B.w | C.w, M packed R' values each.  mask: n_words = ceil(M / 64) words, bit c % 64 of word c / 64 = constraint
// c is broken; lanes beyond M vote 0.  Launched with whole waves.
__global__ void __launch_bounds__(256) k_r1cs_judge(const Fr* __restrict__ rows, uint32_t M, uint32_t n_words,
                                                    unsigned long long* __restrict__ mask)
{
    const uint32_t i    = blockIdx.x * blockDim.x + threadIdx.x;
    bool           fail = false;
    if (i < M) {
        const Fr d = fr9_to_standard(frsub9(frmul9(ld_r9(&rows[i]), ld_r9(&rows[(size_t)M + i])), ld_r9(&rows[2 * (size_t)M + i])));
        fail       = (d.v[0] | d.v[1] | d.v[2] | d.v[3] | d.v[4] | d.v[5] | d.v[6] | d.v[7]) != 0;
    }
    const unsigned long long votes = __ballot(fail);
    if ((threadIdx.x & 63u) == 0 && (i >> 6) < n_words) mask[i >> 6] = votes;
}

// The runs of neighbouring lanes of a wave that hold the same key (here: the same mask word, or the same wire -- the list is
// ordered by wire).  first: the first lane of my run, last: I am its last lane.  Needs the whole wave.
struct WaveRun {
    uint32_t           first;
    bool               last;
    unsigned long long below; // the lanes of my run before me
};
__device__ __forceinline__ WaveRun wave_run(uint32_t key)
{
    const uint32_t           lane  = threadIdx.x & 63u;
    const uint32_t           prev  = __shfl_up(key, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || key != prev);               // first lane of each run (bit 0 is set)
    const unsigned long long upto  = lane == 63u ? ~0ull : (1ull << (lane + 1)) - 1;   // lanes 0 .. lane
    WaveRun                  r;
    r.first = 63u - (uint32_t)__clzll((long long)(heads & upto));
    r.last  = lane == 63u || ((heads >> (lane + 1)) & 1ull) != 0;
    r.below = (upto >> 1) & ~((1ull << r.first) - 1);
    return r;
}
// mask[word] |= the OR of `bits` over each run of lanes that share `word` (a segmented inclusive scan upwards; the run's last lane
// stores).  The mask was cleared before the launch and bits are only ever set: a read that lags behind can only miss bits that
// are set by now -- the atomic is then issued for nothing, the mask is the same.  Other lanes update the word atomically, so the
// read is a relaxed atomic load and `mask` is no __restrict__ pointer: the compiler may not hoist or merge it.
__device__ __forceinline__ void wave_or_into(unsigned long long* mask, uint32_t word, unsigned long long bits)
{
    const uint32_t lane = threadIdx.x & 63u;
    const WaveRun  run  = wave_run(word);
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const unsigned long long up = __shfl_up(bits, d, 64);
        if (lane >= run.first + d) bits |= up;
    }
    if (run.last && bits && (__atomic_load_n(&mask[word], __ATOMIC_RELAXED) & bits) != bits) atomicOr(&mask[word], bits);
}

// The unbound-wire scan.  Change wire i alone by d: the residual a_c b_c - c_c of constraint c moves by d lin + d^2 quad with
//   lin = A^ b_c + B^ a_c - C^,  quad = A^ B^      (A^, B^, C^: the merged coefficients of wire i in constraint c)
// and the wire is bound by c when lin != 0 or quad != 0 (mod r).
// quad: r is prime, so a product of two non-zero residues is non-zero, and r1cs_pairs.h names a coefficient only when its merged
// sum is non-zero: quad != 0 exactly when the incidence names both A^ and B^.  No product is formed for it.
// lin, where quad = 0: at most ONE of A^, B^ is there, so lin is one product (or none) minus C^.  Scalings: a coefficient k is
// stored as k * 2^522 mod r (coef, and side in the same scaling), a sum s lies in rows as the R' value s * 2^261; frmul9 divides
// by 2^261:   frmul9(A^ 2^522, b 2^261) = A^ b 2^522,  frmul9(B^ 2^522, a 2^261) = B^ a 2^522,  and C^ is stored as C^ 2^522
// -- the product and the bare C^ term carry the SAME factor 2^522, so their difference is lin * 2^522.  fr9_to_standard divides
// by 2^261 once more and returns the canonical representative of lin * 2^261: zero exactly when r divides lin (the operands are
// lazy representatives below 2r, as in k_r1cs_judge: only the canonical form tells r from 0).  Bounds: coefficients < r, sums
// < 2r (+ 2^-17 r): the product is < 2r, frsub9 takes a subtrahend < 2r.
// inc / wire: n_pairs incidences ordered by wire (the host leaves wire 0's out, see below).  Positions: < n_entries -> coef,
// n_entries + k -> side[k], R1CS_PAIR_NONE -> 0.
// bound: ceil(n_wires / 64) words, cleared before the launch, bit i = wire i is bound.  The list is ordered by wire, so the
// lanes of a wave whose wires share a mask word are neighbours: their bits are ORed over the wave first and ONE lane per word
// issues the atomicOr, and only where the word does not show the bits yet (atomics on ONE address queue up behind each other
// across the whole device: a wire that sits in a large part of the constraints would cost one per wave); an OR gives the same
// mask whatever order the lanes run in.  Wire 0, the constant, is BOUND by definition: the host leaves its column -- the
// longest of a real circuit -- out of the launch.  Launched with whole waves.
__global__ void __launch_bounds__(256) k_r1cs_incidences(const uint4* __restrict__ inc, const uint32_t* __restrict__ wire,
                                                         uint32_t n_pairs, const Fr* __restrict__ coef, uint32_t n_entries,
                                                         const Fr* __restrict__ side, const Fr* __restrict__ rows, uint32_t M,
                                                         unsigned long long* bound)
{
    const uint32_t i   = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t       w   = 0xffffffffu; // (no wire: the lanes behind the list)
    bool           hit = false;
    if (i < n_pairs) {
        const uint4 e = inc[i]; // x: constraint, y / z / w: positions of A^ / B^ / C^
        w             = wire[i];
        auto at       = [&](uint32_t p) { return ld_r9(p < n_entries ? &coef[p] : &side[p - n_entries]); };
        if (e.y != R1CS_PAIR_NONE && e.z != R1CS_PAIR_NONE) {
            hit = true;
        } else {
            Fr9 lin = fq9_zero();
            if (e.y != R1CS_PAIR_NONE) lin = frmul9(at(e.y), ld_r9(&rows[(size_t)M + e.x]));
            if (e.z != R1CS_PAIR_NONE) lin = frmul9(at(e.z), ld_r9(&rows[e.x]));
            if (e.w != R1CS_PAIR_NONE) lin = frsub9(lin, at(e.w));
            const Fr d = fr9_to_standard(lin);
            hit        = (d.v[0] | d.v[1] | d.v[2] | d.v[3] | d.v[4] | d.v[5] | d.v[6] | d.v[7]) != 0;
        }
    }
    wave_or_into(bound, w >> 6, hit ? 1ull << (w & 63u) : 0ull);
}

// The second-value scan.  With lin and quad as above, an incidence is FREE (lin = quad = 0: every d
// leaves the residual), a PIN (exactly one of them is zero: no d != 0 leaves it -- d lin = 0 or d^2 quad = 0 has the root 0
// alone, r being prime) or a ROOT (neither is zero: d lin + d^2 quad = 0 has exactly one other root, d = -lin / quad).  A wire
// is TWO-VALUED when it has no PIN, at least one ROOT, and all its ROOTs give the same d.
// Scalings, with coefficients k 2^522, sums s 2^261 and frmul9 dividing by 2^261 as above:
//   lin   frmul9(A^ 2^522, b 2^261) + frmul9(B^ 2^522, a 2^261) - C^ 2^522  =  lin 2^522 -- here BOTH of A^, B^ can be there: two
//         products, fradd9 of two values < 2r (its bound is < 4r), then frsub9 with the subtrahend C^ 2^522 < r (its bound is < 2r)
//   quad  frmul9(A^ 2^522, B^ 2^522) = quad 2^783; coefficients < r: the product is < 2r.  quad != 0 exactly when the incidence
//         names both A^ and B^ (see above): the kind needs no product, the comparison and the shift do
//   two ROOTs (lin, quad), (lin0, quad0) give the same d exactly when lin quad0 = lin0 quad (quad, quad0 != 0):
//         frmul9(lin 2^522, quad0 2^783) and frmul9(lin0 2^522, quad 2^783) both carry 2^1044; operands < 2r, products < 2r, and
//         the difference goes through fr9_to_standard: products of coefficients like r - 1 agree only modulo r
//   d     frmul9(quad 2^783, 1) = quad 2^522 = (quad 2^261) 2^261, the R' value of quad 2^261; frinv9 returns the R' value of
//         its inverse, quad^-1 2^-261 2^261 = quad^-1 with factor 1; frmul9(lin 2^522, quad^-1) = (lin / quad) 2^261, an R' value
//         again, negated by frsub9(0, .) -- and fr9_to_standard divides by 2^261: the canonical -lin / quad.
struct IncTerms {
    Fr9  lin;
    bool has_quad; // both A^ and B^ are there: quad != 0
};
// lin 2^522 of incidence e (x: constraint, y / z / w: positions of A^ / B^ / C^)
__device__ __forceinline__ IncTerms inc_terms(const uint4 e, const Fr* __restrict__ coef, uint32_t n_entries,
                                              const Fr* __restrict__ side, const Fr* __restrict__ rows, uint32_t M)
{
    auto     at = [&](uint32_t p) { return ld_r9(p < n_entries ? &coef[p] : &side[p - n_entries]); };
    IncTerms t;
    t.lin      = fq9_zero();
    t.has_quad = e.y != R1CS_PAIR_NONE && e.z != R1CS_PAIR_NONE;
    if (e.y != R1CS_PAIR_NONE) t.lin = frmul9(at(e.y), ld_r9(&rows[(size_t)M + e.x]));
    if (e.z != R1CS_PAIR_NONE) {
        const Fr9 ba = frmul9(at(e.z), ld_r9(&rows[e.x]));
        t.lin        = e.y != R1CS_PAIR_NONE ? fradd9(t.lin, ba) : ba;
    }
    if (e.w != R1CS_PAIR_NONE) t.lin = frsub9(t.lin, at(e.w));
    return t;
}
// quad 2^783 of an incidence that names both
__device__ __forceinline__ Fr9 inc_quad(const uint4 e, const Fr* __restrict__ coef, uint32_t n_entries, const Fr* __restrict__ side)
{
    auto at = [&](uint32_t p) { return ld_r9(p < n_entries ? &coef[p] : &side[p - n_entries]); };
    return frmul9(at(e.y), at(e.z));
}
__device__ __forceinline__ bool fr9_nonzero(const Fr9& x)
{
    const Fr d = fr9_to_standard(x);
    return (d.v[0] | d.v[1] | d.v[2] | d.v[3] | d.v[4] | d.v[5] | d.v[6] | d.v[7]) != 0;
}

// pinned / rooted: ceil(n_wires / 64) words each, cleared before the launch: bit i = wire i has a PIN / a ROOT incidence,
// merged per word and wave as in k_r1cs_incidences.  ref[n_wires], all ones before the launch: the lowest ROOT incidence of each
// wire.  The list is ordered by wire and, within a wire, ascending: among the lanes of a wave that share a wire the FIRST ROOT
// lane holds the wave's minimum, it alone issues the atomicMin, and only where ref does not show an index that low yet (ref only
// ever falls: a read that lags behind costs an atomic for nothing).  One atomic per wire and wave at the most, however long the
// column; a minimum is the same whatever order the lanes run in.  Launched with whole waves.
__global__ void __launch_bounds__(256) k_r1cs_kinds(const uint4* __restrict__ inc, const uint32_t* __restrict__ wire,
                                                    uint32_t n_pairs, const Fr* __restrict__ coef, uint32_t n_entries,
                                                    const Fr* __restrict__ side, const Fr* __restrict__ rows, uint32_t M,
                                                    unsigned long long* pinned, unsigned long long* rooted, uint32_t* ref)
{
    const uint32_t i   = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t       w   = 0xffffffffu; // (no wire: the lanes behind the list)
    bool           pin = false, root = false;
    if (i < n_pairs) {
        w                 = wire[i];
        const IncTerms t  = inc_terms(inc[i], coef, n_entries, side, rows, M);
        const bool     nz = fr9_nonzero(t.lin);
        pin               = nz != t.has_quad;
        root              = nz && t.has_quad;
    }
    const unsigned long long bit = 1ull << (w & 63u);
    wave_or_into(pinned, w >> 6, pin ? bit : 0ull);
    wave_or_into(rooted, w >> 6, root ? bit : 0ull);
    const WaveRun            run   = wave_run(w);
    const unsigned long long roots = __ballot(root);
    if (root && (roots & run.below) == 0 && __atomic_load_n(&ref[w], __ATOMIC_RELAXED) > i) atomicMin(&ref[w], i);
}

// A ROOT incidence other than its wire's reference: lin quad0 = lin0 quad?  Where not, the two move the wire to different
// values and the wire's bit is set in `pinned` (no single d != 0 serves both).  Equality with ONE reference is equality of all
// the d of a wire, since every quad is non-zero.  Nothing per incidence is kept between the kernels: the reference's terms are
// formed again, two products.  Launched with whole waves, after k_r1cs_kinds on the same stream.
__global__ void __launch_bounds__(256) k_r1cs_agree(const uint4* __restrict__ inc, const uint32_t* __restrict__ wire,
                                                    uint32_t n_pairs, const Fr* __restrict__ coef, uint32_t n_entries,
                                                    const Fr* __restrict__ side, const Fr* __restrict__ rows, uint32_t M,
                                                    const uint32_t* __restrict__ ref, unsigned long long* pinned)
{
    const uint32_t i     = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t       w     = 0xffffffffu;
    bool           clash = false;
    if (i < n_pairs) {
        w             = wire[i];
        const uint4 e = inc[i];
        const uint32_t j = ref[w];
        if (e.y != R1CS_PAIR_NONE && e.z != R1CS_PAIR_NONE && j != i && j < n_pairs) {
            const IncTerms t = inc_terms(e, coef, n_entries, side, rows, M);
            if (fr9_nonzero(t.lin)) {
                const uint4    e0 = inc[j];
                const IncTerms t0 = inc_terms(e0, coef, n_entries, side, rows, M);
                clash = fr9_nonzero(frsub9(frmul9(t.lin, inc_quad(e0, coef, n_entries, side)), frmul9(t0.lin, inc_quad(e, coef, n_entries, side))));
            }
        }
    }
    wave_or_into(pinned, w >> 6, clash ? 1ull << (w & 63u) : 0ull);
}

// list[n]: two-valued wires; shift[k] = -lin0 / quad0 of list[k]'s reference incidence, standard form (canonical; non-zero, as
// lin0 != 0).  One inversion per lane: the work is the list's, not the circuit's.
__global__ void __launch_bounds__(64) k_r1cs_shifts(const uint32_t* __restrict__ list, uint32_t n, const uint4* __restrict__ inc,
                                                    uint32_t n_pairs, const Fr* __restrict__ coef, uint32_t n_entries,
                                                    const Fr* __restrict__ side, const Fr* __restrict__ rows, uint32_t M,
                                                    const uint32_t* __restrict__ ref, Fr* __restrict__ shift)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t j = ref[list[k]];
    if (j >= n_pairs) return; // (a listed wire has a ROOT incidence)
    const uint4    e0 = inc[j];
    const IncTerms t0 = inc_terms(e0, coef, n_entries, side, rows, M);
    Fr9            one = fq9_zero();
    one.l[0]           = 1;
    const Fr9 qinv = frinv9(frmul9(inc_quad(e0, coef, n_entries, side), one));
    st_fr(&shift[k], fr9_to_standard(frsub9(fq9_zero(), frmul9(t0.lin, qinv))));
}

// The determinism closure (k16_r1cs_determined_wires): the least set K of wires that holds the seed and
// is closed under
//     constraint c is not broken, exactly ONE wire x with a non-zero merged coefficient in c lies outside K, and the
//     incidence (x, c) is a PIN  ==>  x joins K
// computed level by level (K_0 = seed, K_k+1 = K_k and what the rule gives with respect to K_k): round[x] is the first level
// that holds x, by[x] the lowest constraint that gave it there.  Any witness that satisfies the circuit and agrees with this one
// on the seed agrees with it on K: in c every wire but x is equal, so the residuals differ by t lin + t^2 quad, both residuals
// are 0, and a PIN leaves t = 0 alone.  Three details of the rule carry that argument -- none of them is an inefficiency:
//   a BROKEN constraint derives nothing     its residual under this witness is not 0, the difference says nothing about t
//   a FREE incidence of an outside wire still COUNTS as an outside wire     two outside wires x, y move the residual by a cross
//                                           term dx dy (A^x B^y + A^y B^x) that neither wire's lin or quad shows
//   a ROOT derives nothing                  t = -lin / quad is the second solution: the two-valued case
// Each constraint carries two words: cnt[c], the number of its incidences (of the device list: wire 0, always in K, is not on
// it) whose wire lies outside K, and xr[c], the XOR of those incidences' indices -- where cnt is 1, xr IS the one outside
// incidence.  No constraint-ordered copy of the list is needed.
//   k_r1cs_det_init    one lane per incidence: a wire outside the seed counts into cnt / xr of its constraint
//   k_r1cs_det_first   one lane per constraint: cnt = 1 -> the candidate list
//   k_r1cs_det_derive  one lane per candidate of this round: not broken, cnt still 1 (a constraint may have fallen on to 0 in
//                      the expansion that listed it), the outside incidence a PIN -> atomicMin(by[x], c); the lane that found
//                      by[x] empty appends x to the frontier.  `known` is only read here, so by[x] ends as the minimum over
//                      exactly the constraints that qualify with respect to the level before
//   k_r1cs_det_expand  one lane per frontier wire: known bit, round[x], and for each incidence of its column cnt[c] -= 1,
//                      xr[c] ^= index; the lane that saw cnt fall from 2 to 1 appends c to the candidates -- once per
//                      constraint, cnt only ever falls.  A column of up to DET_SHORT incidences is walked by its lane, a longer
//                      one by the whole wave, 64 incidences a step: no lane's work grows with a column's length.
// Both lists only grow: every constraint becomes a candidate at most once and is judged once (its kind depends on the witness
// alone: a candidate that is no PIN now never is), every wire enters the frontier at most once; a round is a range of each.  The
// host reads both list sizes once per round from a record in pinned, device-mapped memory, written by the last workgroup of
// k_r1cs_det_first / _expand to finish (a ticket per workgroup; nothing waits).  Appends are one atomicAdd per wave and list.
// The order inside a list is arbitrary and nothing observable depends on it: masks are ORs, by is a minimum, round has one value
// per wire, cnt is a sum and xr an XOR, the sizes are sums.
constexpr uint32_t DET_NONE  = 0xffffffffu;
constexpr uint32_t DET_SHORT = 8;
constexpr uint32_t DET_GRID  = 512; // workgroups of a kernel that ends in det_publish
struct DetState {
    uint32_t n_front, n_cand; // sizes of the two lists
    uint32_t done, pad;       // workgroups of the running kernel that have finished
};
struct DetRecord {
    uint32_t n_front, n_cand;
};

// list[*total ...] <- value of the lanes that `have` one: one atomicAdd per wave.  Needs the whole wave.  cap: the list's room
// (every constraint / wire is appended once at the most, so it is never reached).
__device__ __forceinline__ void wave_append(uint32_t* __restrict__ list, uint32_t* total, uint32_t cap, bool have, uint32_t value)
{
    const unsigned long long votes = __ballot(have);
    if (!votes) return;
    const uint32_t lane   = threadIdx.x & 63u;
    const int      leader = __ffsll((long long)votes) - 1;
    uint32_t       base   = 0;
    if ((int)lane == leader) base = atomicAdd(total, (uint32_t)__popcll(votes));
    base               = __shfl(base, leader, 64);
    const uint32_t pos = base + (uint32_t)__popcll(votes & ((1ull << lane) - 1));
    if (have && pos < cap) list[pos] = value;
}
// The last workgroup to get here copies the list sizes into the host's record.  Every lane of the workgroup calls it, after its
// last append.
__device__ __forceinline__ void det_publish(DetState* st, DetRecord* rec)
{
    __syncthreads();
    if (threadIdx.x != 0) return;
    __threadfence(); // this workgroup's appends before its ticket
    if (atomicAdd(&st->done, 1u) != gridDim.x - 1) return;
    __threadfence(); // every other workgroup's ticket before the reads
    rec->n_front = __atomic_load_n(&st->n_front, __ATOMIC_RELAXED);
    rec->n_cand  = __atomic_load_n(&st->n_cand, __ATOMIC_RELAXED);
    st->done     = 0; // (the next launch on the stream starts behind this kernel)
}
__device__ __forceinline__ bool det_bit(const unsigned long long* __restrict__ mask, uint32_t i) { return (mask[i >> 6] >> (i & 63u)) & 1ull; }

// cnt / xr: M words each, cleared before the launch.  seed: ceil(n_wires / 64) words.
__global__ void __launch_bounds__(256) k_r1cs_det_init(const uint4* __restrict__ inc, const uint32_t* __restrict__ wire,
                                                       uint32_t n_pairs, uint32_t n_wires, uint32_t M,
                                                       const unsigned long long* __restrict__ seed, uint32_t* cnt, uint32_t* xr)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs) return;
    const uint32_t w = wire[i], c = inc[i].x;
    if (w >= n_wires || c >= M || det_bit(seed, w)) return;
    atomicAdd(&cnt[c], 1u);
    atomicXor(&xr[c], i);
}

// Launched with whole waves, DET_GRID workgroups at the most: a workgroup strides the constraints (every workgroup draws a ticket
// in det_publish, on ONE counter: a ticket per 256 constraints would cost more than the pass).
__global__ void __launch_bounds__(256) k_r1cs_det_first(const uint32_t* __restrict__ cnt, uint32_t M, uint32_t* __restrict__ cand,
                                                        DetState* st, DetRecord* rec)
{
    for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < M; base += (uint64_t)gridDim.x * 256u) { // (the same trips for a whole workgroup)
        const uint64_t c = base + threadIdx.x;
        wave_append(cand, &st->n_cand, M, c < M && cnt[c] == 1u, (uint32_t)c);
    }
    det_publish(st, rec);
}

// cand[0 .. n): the candidates of this round.  verdict: the check's mask (bit c: constraint c is broken).  Launched with whole waves.
__global__ void __launch_bounds__(256) k_r1cs_det_derive(const uint32_t* __restrict__ cand, uint32_t n, const uint4* __restrict__ inc,
                                                         const uint32_t* __restrict__ wire, uint32_t n_pairs,
                                                         const Fr* __restrict__ coef, uint32_t n_entries, const Fr* __restrict__ side,
                                                         const Fr* __restrict__ rows, uint32_t M,
                                                         const unsigned long long* __restrict__ verdict,
                                                         const unsigned long long* __restrict__ known, const uint32_t* __restrict__ cnt,
                                                         const uint32_t* __restrict__ xr, uint32_t n_wires, uint32_t* by,
                                                         uint32_t* __restrict__ front, DetState* st)
{
    const uint32_t k   = blockIdx.x * blockDim.x + threadIdx.x;
    bool           add = false;
    uint32_t       x   = 0;
    if (k < n) {
        const uint32_t c = cand[k];
        if (c < M && !det_bit(verdict, c) && cnt[c] == 1u) {
            const uint32_t idx = xr[c];
            if (idx < n_pairs) {
                x = wire[idx];
                if (x < n_wires && !det_bit(known, x)) {
                    const IncTerms t = inc_terms(inc[idx], coef, n_entries, side, rows, M);
                    if (fr9_nonzero(t.lin) != t.has_quad) add = atomicMin(&by[x], c) == DET_NONE; // a PIN
                }
            }
        }
    }
    wave_append(front, &st->n_front, n_wires, add, x);
}

// front[from .. st->n_front): the wires this round derived (the size is final: k_r1cs_det_derive has ended); a workgroup strides
// them, so any grid covers them.  start[i] .. start[i + 1]: the column of wire i in inc.  Launched with whole waves, DET_GRID
// workgroups at the most (the tickets of det_publish, as in k_r1cs_det_first).
__global__ void __launch_bounds__(256) k_r1cs_det_expand(const uint32_t* __restrict__ front, uint32_t from, uint32_t round,
                                                         const uint32_t* __restrict__ start, const uint4* __restrict__ inc,
                                                         uint32_t n_pairs, uint32_t n_wires, uint32_t M, unsigned long long* known,
                                                         uint32_t* __restrict__ round_of, uint32_t* cnt, uint32_t* xr,
                                                         uint32_t* __restrict__ cand, DetState* st, DetRecord* rec)
{
    const uint32_t lane  = threadIdx.x & 63u;
    const uint32_t total = __atomic_load_n(&st->n_front, __ATOMIC_RELAXED);
    const uint32_t todo  = total > from ? total - from : 0; // (the same in every lane: whole workgroups take the same trips)
    for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < todo; base += (uint64_t)gridDim.x * 256u) {
        const uint64_t k = base + threadIdx.x;
        uint32_t       x = DET_NONE, s = 0, e = 0;
        if (k < todo) {
            const uint32_t f = front[from + k];
            if (f < n_wires) {
                x           = f;
                round_of[x] = round;
                s           = start[x];
                e           = min(start[x + 1], n_pairs);
            }
        }
        wave_or_into(known, x >> 6, x != DET_NONE ? 1ull << (x & 63u) : 0ull);
        // one incidence: leaves the outside count of its constraint
        auto leave = [&](bool act, uint32_t idx) {
            bool     listed = false;
            uint32_t c      = 0;
            if (act) {
                c = inc[idx].x;
                if (c < M) {
                    listed = atomicSub(&cnt[c], 1u) == 2u;
                    atomicXor(&xr[c], idx);
                }
            }
            wave_append(cand, &st->n_cand, M, listed, c);
        };
        const uint32_t len = e > s ? e - s : 0;
        for (uint32_t j = 0; j < DET_SHORT; j++) {
            const bool act = len <= DET_SHORT && j < len;
            if (!__ballot(act)) break;
            leave(act, s + j);
        }
        unsigned long long longs = __ballot(len > DET_SHORT);
        while (longs) {
            const int src = __ffsll((long long)longs) - 1;
            longs &= longs - 1;
            const uint32_t ls = __shfl(s, src, 64), le = __shfl(e, src, 64);
            for (uint64_t at = ls; at < le; at += 64u) leave(at + lane < le, (uint32_t)(at + lane));
        }
    }
    det_publish(st, rec);
}

// What a prove call keeps of its check (pinned, device-mapped; read by the host after the check is joined).
struct CheckRecord {
    unsigned long long flags;                    // WTNS_* of k_r1cs_wtns
    unsigned long long count;                    // exact number of broken constraints
    uint32_t           lowest[K16_R1CS_REPORT_MAX]; // the lowest min(count, K16_R1CS_REPORT_MAX) of them, ascending
};

// mask[n_words] | flags -> rec.  ONE workgroup of 256 lanes walks the mask in tiles of 256 words (16384 constraints), a word per
// lane: popcount, an ordered scan over the tile (shuffles inside a wave, the four wave totals through LDS) on top of the
// running total of the tiles before gives every word the rank of its first set bit; a word whose rank is below
// K16_R1CS_REPORT_MAX writes its bits' numbers at rank, rank + 1, ... -- every slot of the list has exactly one writer,
// whatever the order the lanes run in.  The tile of the next round is loaded before this round's scan.
__global__ void __launch_bounds__(256) k_r1cs_summary(const unsigned long long* __restrict__ mask, uint32_t n_words,
                                                      CheckRecord* __restrict__ rec)
{
    __shared__ uint32_t wave_total[2][4]; // (two sets, by the tile's parity: one barrier a tile)
    const uint32_t      lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long  running = 0; // broken constraints in the tiles before this one (the same in every lane)
    unsigned long long  next    = threadIdx.x < n_words ? mask[threadIdx.x] : 0ull;
    for (uint32_t base = 0; base < n_words; base += 256u) {
        const uint32_t           w = base + threadIdx.x;
        const unsigned long long m = next;
        next                       = w + 256u < n_words ? mask[w + 256u] : 0ull; // (n_words <= 2^26: no wrap)
        const uint32_t mine = (uint32_t)__popcll(m);
        uint32_t       incl = mine; // inclusive scan over the wave
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        uint32_t* totals = wave_total[(base >> 8) & 1u];
        if (lane == 63u) totals[wave] = incl;
        __syncthreads(); // (a wave writes this set again two tiles on: every wave has passed the next tile's barrier by then)
        uint32_t before = 0, tile = 0;
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t t = totals[k];
            if (k < wave) before += t;
            tile += t;
        }
        unsigned long long rank = running + before + (incl - mine);
        unsigned long long bits = m;
        while (bits && rank < (unsigned long long)K16_R1CS_REPORT_MAX) {
            rec->lowest[rank++] = w * 64u + (uint32_t)__ffsll((long long)bits) - 1u;
            bits &= bits - 1;
        }
        running += tile;
    }
    if (threadIdx.x == 0) {
        rec->flags = mask[n_words];
        rec->count = running;
    }
}

} // namespace

struct k16_r1cs {
    k16_ctx* ctx = nullptr;
    R1csFile file; // the host copy: k16_r1cs_match_zkey compares it with a key
    uint32_t n_wires = 0, n_public = 0, M = 0, n_words = 0;
    // the circuit on the device (see k_r1cs_rows)
    SpmvSlice* d_slices = nullptr;
    SpmvLong*  d_longs  = nullptr;
    uint32_t * d_rowof = nullptr, *d_wire = nullptr;
    Fr*        d_coef  = nullptr; // coefficient * 2^522 mod r, as the prover stores its own
    uint32_t   n_slices = 0, n_long = 0;
    uint64_t   n_entries = 0; // of the plan d_coef was laid out by (r1cs_pairs.h names coefficients by position in it)
    // per check
    Fr*                 d_wtns = nullptr; // an uploaded witness (k16_r1cs_check_mem / _file)
    uint16_t*           d_n16  = nullptr;
    Fr*                 d_rows = nullptr; // [3 M]
    unsigned long long* d_mask = nullptr; // [n_words] verdicts | [1] witness flags
    unsigned long long* h_mask = nullptr; // pinned copy
    bool                have_values = false; // d_rows holds the sums of a completed check (k16_r1cs_last_values)
    // attached to a prover (k16_r1cs_attach): made by the first attach, kept until the object goes
    CheckRecord *h_rec = nullptr, *d_rec = nullptr; // pinned, device-mapped
    hipStream_t  forked_on = nullptr; // the prover's stream a check is (or may be) in flight on; null: none
    // the unbound-wire scan: the list by the first call that needs it, the device side by the first scan; kept until the object goes
    std::unique_ptr<R1csPairs> pairs;
    uint4*                     d_inc     = nullptr; // R1csPair of every incidence of the wires 1 .. n_wires - 1
    uint32_t*                  d_incwire = nullptr; // their wires
    Fr*                        d_side    = nullptr; // merged sums * 2^522 mod r
    unsigned long long *       d_bound = nullptr, *h_bound = nullptr; // [ceil(n_wires / 64)], device / pinned
    bool                       scan_ready = false;
    // the second-value scan, on top of the list above: made by its first call, kept until the object goes
    unsigned long long *d_kinds = nullptr, *h_kinds = nullptr; // pinned | rooted, [ceil(n_wires / 64)] each, device / pinned
    uint32_t*           d_ref   = nullptr;                     // [n_wires] the lowest ROOT incidence of each wire
    uint32_t *          d_list = nullptr, *h_list = nullptr;   // [n_wires] the listed wires, device / pinned
    Fr*                 d_shift = nullptr;                     // [n_wires] their shifts, standard form
    bool                second_ready = false;
    // the determinism closure, on top of the same list: made by its first call, kept until the object goes
    uint32_t*           d_det_start = nullptr;                     // [n_wires + 1] the columns of the device list
    unsigned long long *d_det_masks = nullptr, *h_det_masks = nullptr; // seed | known, [ceil(n_wires / 64)] each, device / pinned
    uint32_t*           d_det_cnt   = nullptr;                     // cnt | xr, [M] each
    uint32_t*           d_det_by    = nullptr;                     // by | round, [n_wires] each
    uint32_t *          d_det_cand = nullptr, *d_det_front = nullptr; // [M] / [n_wires]: the two lists
    DetState*           d_det_state = nullptr;
    DetRecord *         h_det_rec = nullptr, *d_det_rec = nullptr; // pinned, device-mapped
    bool                det_ready = false;
};

void k16_r1cs_view(const k16_r1cs* r, k16_ctx** ctx, const R1csFile** file)
{
    *ctx  = r->ctx;
    *file = &r->file;
}

// the scan's device side (the host list stays)
static void r1cs_scan_free(k16_r1cs* r)
{
    void* bufs[] = {r->d_inc, r->d_incwire, r->d_side, r->d_bound};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    if (r->h_bound) (void)hipHostFree(r->h_bound);
    r->d_inc = nullptr, r->d_incwire = nullptr, r->d_side = nullptr, r->d_bound = nullptr, r->h_bound = nullptr;
    r->scan_ready = false;
}

static void r1cs_second_free(k16_r1cs* r)
{
    void* bufs[] = {r->d_kinds, r->d_ref, r->d_list, r->d_shift};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    if (r->h_kinds) (void)hipHostFree(r->h_kinds);
    if (r->h_list) (void)hipHostFree(r->h_list);
    r->d_kinds = nullptr, r->h_kinds = nullptr, r->d_ref = nullptr, r->d_list = nullptr, r->h_list = nullptr, r->d_shift = nullptr;
    r->second_ready = false;
}

static void r1cs_det_free(k16_r1cs* r)
{
    void* bufs[] = {r->d_det_start, r->d_det_masks, r->d_det_cnt, r->d_det_by, r->d_det_cand, r->d_det_front, r->d_det_state};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    if (r->h_det_masks) (void)hipHostFree(r->h_det_masks);
    if (r->h_det_rec) (void)hipHostFree(r->h_det_rec);
    r->d_det_start = nullptr, r->d_det_masks = nullptr, r->h_det_masks = nullptr, r->d_det_cnt = nullptr, r->d_det_by = nullptr;
    r->d_det_cand = nullptr, r->d_det_front = nullptr, r->d_det_state = nullptr, r->h_det_rec = nullptr, r->d_det_rec = nullptr;
    r->det_ready = false;
}

static void r1cs_free(k16_r1cs* r)
{
    if (!r) return;
    if (r->ctx) (void)hipSetDevice(r->ctx->device);
    r1cs_det_free(r);
    r1cs_second_free(r);
    r1cs_scan_free(r);
    void* bufs[] = {r->d_slices, r->d_longs, r->d_rowof, r->d_wire, r->d_coef, r->d_wtns, r->d_n16, r->d_rows, r->d_mask};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    if (r->h_mask) (void)hipHostFree(r->h_mask);
    if (r->forked_on) (void)hipStreamSynchronize(r->forked_on);
    if (r->h_rec) (void)hipHostFree(r->h_rec);
    delete r;
}

#define K16_HIP_R(ctx, call, r)                                             \
    do {                                                                    \
        hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess) {                                             \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_); \
            (void)hipStreamSynchronize((ctx)->stream); /* uploads from local vectors may be queued */ \
            r1cs_free(r);                                                   \
            return K16_ERR_HIP;                                             \
        }                                                                   \
    } while (0)

extern "C" int k16_r1cs_create_mem(k16_ctx* ctx, const void* r1cs, size_t size, k16_r1cs** out)
{
    return k16_guard(ctx, [&]() -> int {
    if (!ctx || !r1cs || !out) return K16_ERR_ARG;
    *out = nullptr;
    std::unique_ptr<k16_r1cs> holder(new k16_r1cs()); // (plain members only until the device buffers exist)
    k16_r1cs*                 r = holder.get();
    const char*               why = "";
    int                       rc  = r1cs_parse((const uint8_t*)r1cs, size, &r->file, &why);
    if (rc) {
        ctx->err = why;
        return rc;
    }
    R1csPlan plan;
    if ((rc = r1cs_plan_build(r->file, &plan))) {
        ctx->err = "r1cs: too many terms for 32-bit entry offsets";
        return rc;
    }
    r->n_wires  = r->file.n_wires;
    r->n_public = r->file.n_public();
    r->M        = r->file.n_constraints;
    r->n_words  = (uint32_t)(((uint64_t)r->M + 63) / 64);
    r->n_slices = plan.plan.n_slices;
    r->n_long   = plan.plan.n_long;
    r->n_entries = plan.plan.n_entries;
    const uint64_t        n_entries = std::max<uint64_t>(plan.plan.n_entries, 1);
    std::vector<uint32_t> wire(n_entries, 0);
    std::vector<R1csFr>   vals(n_entries, R1csFr{{0, 0, 0, 0}}); // padding: coefficient 0 (times wire 0)
    const R1csScale       to_r9(522);
    for (uint64_t t = 0; t < r->file.n_terms(); t++) {
        wire[plan.pos[t]] = r->file.wire[t];
        vals[plan.pos[t]] = to_r9(r->file.coef[t]);
    }
    r->ctx = ctx;
    holder.release(); // from here on r1cs_free owns it
    K16_HIP_R(ctx, hipSetDevice(ctx->device), r);
    const SpmvPlan& pl = plan.plan;
    K16_HIP_R(ctx, hipMalloc((void**)&r->d_slices, pl.slices.size() * sizeof(SpmvSlice)), r);
    K16_HIP_R(ctx, hipMalloc((void**)&r->d_longs, pl.longs.size() * sizeof(SpmvLong)), r);
    K16_HIP_R(ctx, hipMalloc((void**)&r->d_rowof, pl.row_of.size() * 4), r);
    K16_HIP_R(ctx, hipMalloc((void**)&r->d_wire, wire.size() * 4), r);
    K16_HIP_R(ctx, hipMalloc((void**)&r->d_coef, vals.size() * 32), r);
    K16_HIP_R(ctx, hipMalloc((void**)&r->d_wtns, (size_t)r->n_wires * 32), r);
    K16_HIP_R(ctx, hipMalloc((void**)&r->d_n16, (size_t)r->n_wires * 2 + 64), r);
    K16_HIP_R(ctx, hipMalloc((void**)&r->d_rows, std::max<size_t>(3 * (size_t)r->M, 1) * 32), r);
    K16_HIP_R(ctx, hipMalloc((void**)&r->d_mask, ((size_t)r->n_words + 1) * 8), r);
    K16_HIP_R(ctx, hipHostMalloc((void**)&r->h_mask, ((size_t)r->n_words + 1) * 8, hipHostMallocDefault), r);
    hipStream_t st = ctx->stream;
    K16_HIP_R(ctx, hipMemcpyAsync(r->d_slices, pl.slices.data(), pl.slices.size() * sizeof(SpmvSlice), hipMemcpyHostToDevice, st), r);
    K16_HIP_R(ctx, hipMemcpyAsync(r->d_longs, pl.longs.data(), pl.longs.size() * sizeof(SpmvLong), hipMemcpyHostToDevice, st), r);
    K16_HIP_R(ctx, hipMemcpyAsync(r->d_rowof, pl.row_of.data(), pl.row_of.size() * 4, hipMemcpyHostToDevice, st), r);
    K16_HIP_R(ctx, hipMemcpyAsync(r->d_wire, wire.data(), wire.size() * 4, hipMemcpyHostToDevice, st), r);
    K16_HIP_R(ctx, hipMemcpyAsync(r->d_coef, vals.data(), vals.size() * 32, hipMemcpyHostToDevice, st), r);
    K16_HIP_R(ctx, hipStreamSynchronize(st), r);
    *out = r;
    return K16_OK;
    });
}

extern "C" int k16_r1cs_create(k16_ctx* ctx, const char* path, k16_r1cs** out)
{
    return k16_guard(ctx, [&]() -> int {
    if (!ctx || !path || !out) return K16_ERR_ARG;
    *out = nullptr;
    return k16_file_apply(ctx, path, "r1cs", [&](const uint8_t* base, size_t size) { return k16_r1cs_create_mem(ctx, base, size, out); });
    });
}

extern "C" void k16_r1cs_destroy(k16_r1cs* r)
{
    k16_guard_void([&]() {
        if (r && r->ctx && r->ctx->stream) (void)hipStreamSynchronize(r->ctx->stream);
        r1cs_free(r);
    });
}

extern "C" int k16_r1cs_info(const k16_r1cs* r, uint32_t* n_wires, uint32_t* n_public, uint32_t* n_constraints, uint64_t* n_terms)
{
    if (!r) return K16_ERR_ARG;
    if (n_wires) *n_wires = r->n_wires;
    if (n_public) *n_public = r->n_public;
    if (n_constraints) *n_constraints = r->M;
    if (n_terms) *n_terms = r->file.n_terms();
    return K16_OK;
}

// The three kernels of a check on st: d_wtns holds n_wires values; d_n16 their 16-bit words, or null when this call is to make
// them (into r->d_n16).
static int r1cs_launch(k16_ctx* ctx, k16_r1cs* r, const Fr* d_wtns, const uint16_t* d_n16, hipStream_t st)
{
    K16_HIP(ctx, hipMemsetAsync(r->d_mask + r->n_words, 0, 8, st));
    hipLaunchKernelGGL(k_r1cs_wtns, dim3((r->n_wires + 255) / 256), dim3(256), 0, st, (const uint4*)d_wtns, r->n_wires,
                       d_n16 ? nullptr : r->d_n16, r->d_mask + r->n_words);
    if (r->M) {
        const uint64_t waves = (uint64_t)r->n_slices + r->n_long;
        {
            k16_stat_scope sc(ctx, "r1cs_rows", st);
            hipLaunchKernelGGL(k_r1cs_rows, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, r->d_slices, r->n_slices, r->d_rowof,
                               r->d_longs, r->n_long, r->d_wire, r->d_coef, d_wtns, d_n16 ? d_n16 : r->d_n16, r->d_rows);
        }
        {
            k16_stat_scope sc(ctx, "r1cs_judge", st);
            hipLaunchKernelGGL(k_r1cs_judge, dim3((r->M + 255) / 256), dim3(256), 0, st, r->d_rows, r->M, r->n_words, r->d_mask);
        }
    }
    K16_HIP(ctx, hipGetLastError());
    return K16_OK;
}

// The check proper, on the context's stream.  Whatever fails, the stream is drained before the caller returns.
static int r1cs_enqueue(k16_ctx* ctx, k16_r1cs* r, const Fr* d_wtns, const uint16_t* d_n16)
{
    hipStream_t st = ctx->stream;
    const int   rc = r1cs_launch(ctx, r, d_wtns, d_n16, st);
    if (rc) return rc;
    K16_HIP(ctx, hipMemcpyAsync(r->h_mask, r->d_mask, ((size_t)r->n_words + 1) * 8, hipMemcpyDeviceToHost, st));
    K16_HIP(ctx, hipStreamSynchronize(st));
    return K16_OK;
}

// ---- the check under a proof (ctx.h; prover.hip k16_prover_set_r1cs)
int k16_r1cs_attach(k16_r1cs* r, k16_ctx* ctx, uint32_t n_vars, uint32_t n_public)
{
    if (r->ctx != ctx || r->n_wires != n_vars || r->n_public != n_public) {
        ctx->err = r->ctx != ctx            ? "k16_prover_set_r1cs: the R1CS object belongs to another context"
                   : r->n_wires != n_vars ? "k16_prover_set_r1cs: the circuit's wire count is not the proving key's nVars"
                                          : "k16_prover_set_r1cs: the circuit's public wire count is not the proving key's nPublic";
        return K16_ERR_ARG;
    }
    K16_HIP(ctx, hipSetDevice(ctx->device));
    if (!r->h_rec) {
        K16_HIP(ctx, hipHostMalloc((void**)&r->h_rec, sizeof(CheckRecord), hipHostMallocMapped | hipHostMallocCoherent));
        K16_HIP(ctx, hipHostGetDevicePointer((void**)&r->d_rec, r->h_rec, 0));
    }
    return K16_OK;
}

int k16_r1cs_fork(k16_r1cs* r, hipStream_t st, const Fr* d_wtns, const uint16_t* d_n16)
{
    k16_ctx* ctx   = r->ctx;
    r->have_values = false;
    r->forked_on   = st;
    const int rc   = r1cs_launch(ctx, r, d_wtns, d_n16, st);
    if (rc) return rc;
    {
        k16_stat_scope sc(ctx, "r1cs_summary", st);
        hipLaunchKernelGGL(k_r1cs_summary, dim3(1), dim3(256), 0, st, r->d_mask, r->n_words, r->d_rec);
    }
    K16_HIP(ctx, hipGetLastError());
    return K16_OK;
}

void k16_r1cs_drain(k16_r1cs* r)
{
    if (r->forked_on) (void)hipStreamSynchronize(r->forked_on);
    r->forked_on = nullptr;
}

int k16_r1cs_join(k16_r1cs* r, int* status, uint64_t* n_failed, uint32_t* lowest)
{
    k16_ctx* ctx = r->ctx;
    *status      = K16_CHECK_NONE;
    *n_failed    = 0;
    if (!r->forked_on) return K16_OK;
    hipStream_t st = r->forked_on;
    r->forked_on   = nullptr;
    K16_HIP(ctx, hipStreamSynchronize(st));
    const CheckRecord* rec = r->h_rec;
    if (rec->flags) {
        *status = K16_CHECK_WITNESS_REFUSED;
        return K16_OK;
    }
    r->have_values = true;
    *n_failed      = rec->count;
    *status        = rec->count ? K16_CHECK_BROKEN : K16_CHECK_SATISFIED;
    const uint64_t n = std::min<uint64_t>(rec->count, K16_R1CS_REPORT_MAX);
    for (uint64_t k = 0; k < n; k++) lowest[k] = rec->lowest[k];
    return K16_OK;
}

static int r1cs_check(k16_ctx* ctx, k16_r1cs* r, const Fr* d_wtns, const uint16_t* d_n16, uint64_t* n_failed, uint32_t* h_failed,
                      uint32_t cap)
{
    *n_failed      = 0;
    r->have_values = false;
    const int rc   = r1cs_enqueue(ctx, r, d_wtns, d_n16);
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream); // nothing of the check stays in flight
        return rc;
    }
    const unsigned long long flags = r->h_mask[r->n_words];
    if (flags) {
        ctx->err = (flags & WTNS_NOT_BELOW_R) ? "witness: a wire value is not below r" : "witness: wire 0 is not 1";
        return K16_ERR_FORMAT;
    }
    r->have_values = true;
    uint64_t count = 0;
    for (uint32_t w = 0; w < r->n_words; w++) {
        unsigned long long m = r->h_mask[w];
        while (m) {
            const uint32_t c = w * 64u + (uint32_t)__builtin_ctzll(m);
            if (h_failed && count < cap) h_failed[count] = c;
            count++;
            m &= m - 1;
        }
    }
    *n_failed = count;
    return K16_OK;
}

static int r1cs_check_host(k16_ctx* ctx, k16_r1cs* r, const void* h_wtns, uint64_t* n_failed, uint32_t* h_failed, uint32_t cap)
{
    K16_HIP(ctx, hipSetDevice(ctx->device));
    K16_HIP(ctx, hipMemcpyAsync(r->d_wtns, h_wtns, (size_t)r->n_wires * 32, hipMemcpyHostToDevice, ctx->stream));
    return r1cs_check(ctx, r, r->d_wtns, nullptr, n_failed, h_failed, cap);
}

extern "C" int k16_r1cs_check_mem(k16_ctx* ctx, k16_r1cs* r, const void* h_wtns, uint64_t n_wires, uint64_t* n_failed,
                                  uint32_t* h_failed, uint32_t cap)
{
    return k16_guard(ctx, [&]() -> int {
    if (!ctx || !r || !h_wtns || !n_failed || r->ctx != ctx) return K16_ERR_ARG;
    *n_failed = 0;
    if (n_wires != r->n_wires) {
        ctx->err = "witness does not have as many values as the circuit has wires";
        return K16_ERR_ARG;
    }
    return r1cs_check_host(ctx, r, h_wtns, n_failed, h_failed, cap);
    });
}

extern "C" int k16_r1cs_check_file(k16_ctx* ctx, k16_r1cs* r, const char* wtns_path, uint64_t* n_failed, uint32_t* h_failed,
                                   uint32_t cap)
{
    return k16_guard(ctx, [&]() -> int {
    if (!ctx || !r || !wtns_path || !n_failed || r->ctx != ctx) return K16_ERR_ARG;
    *n_failed = 0;
    return k16_wtns_file_apply(ctx, wtns_path, [&](const uint8_t* values, uint64_t have) -> int {
        if (have != r->n_wires) {
            ctx->err = "wtns: the file does not hold as many values as the circuit has wires";
            return K16_ERR_FORMAT;
        }
        return r1cs_check_host(ctx, r, values, n_failed, h_failed, cap);
    });
    });
}

extern "C" int k16_r1cs_check_prover_witness(k16_prover* p, k16_r1cs* r, uint64_t* n_failed, uint32_t* h_failed, uint32_t cap)
{
    if (!p || !r || !n_failed) return K16_ERR_ARG;
    *n_failed = 0;
    return k16_guard(r->ctx, [&]() -> int {
    k16_ctx*        ctx    = nullptr;
    const Fr*       d_wtns = nullptr;
    const uint16_t* d_n16  = nullptr;
    uint32_t        n_vars = 0;
    const int       rc     = k16_prover_witness_view(p, &ctx, &d_wtns, &d_n16, &n_vars);
    if (r->ctx != ctx) {
        ctx->err = "the R1CS object must live on the prover's context";
        return K16_ERR_ARG;
    }
    if (n_vars != r->n_wires) {
        ctx->err = "the circuit's wire count is not the proving key's";
        return K16_ERR_ARG;
    }
    if (rc) return rc;
    K16_HIP(ctx, hipSetDevice(ctx->device));
    return r1cs_check(ctx, r, d_wtns, d_n16, n_failed, h_failed, cap);
    });
}

extern "C" int k16_r1cs_last_values(k16_r1cs* r, uint32_t constraint, void* h_out96)
{
    return k16_guard(r ? r->ctx : nullptr, [&]() -> int {
    if (!r || !h_out96) return K16_ERR_ARG;
    k16_ctx* ctx = r->ctx;
    if (!r->have_values || constraint >= r->M) {
        ctx->err = r->have_values ? "constraint number out of range" : "no completed check to read values from";
        return K16_ERR_ARG;
    }
    K16_HIP(ctx, hipSetDevice(ctx->device));
    Fr packed[3];
    for (int m = 0; m < 3; m++)
        K16_HIP(ctx, hipMemcpyAsync(&packed[m], r->d_rows + (size_t)m * r->M + constraint, 32, hipMemcpyDeviceToHost, ctx->stream));
    K16_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int m = 0; m < 3; m++) {
        const Fr v = fr9_to_standard(fr9_load(packed[m].v)); // the same host code the device runs
        memcpy((uint8_t*)h_out96 + 32 * m, v.v, 32);
    }
    return K16_OK;
    });
}

// ---- the unbound-wire scan
// The incidence list, made once.  K16_ERR_ARG: 2^32 incidences or more.
static int r1cs_pairs_get(k16_ctx* ctx, k16_r1cs* r)
{
    if (r->pairs) return K16_OK;
    R1csPlan plan; // the layout k16_r1cs_create_mem uploaded: r1cs_plan_build is a function of the file alone
    if (r1cs_plan_build(r->file, &plan)) {
        ctx->err = "r1cs: too many terms for 32-bit entry offsets";
        return K16_ERR_ARG;
    }
    if (plan.plan.n_entries != r->n_entries) { // positions would point into another layout than d_coef's
        ctx->err = "r1cs: the rebuilt plan is not the one the coefficients were uploaded by";
        return K16_ERR_ARG;
    }
    std::unique_ptr<R1csPairs> p(new R1csPairs());
    if (r1cs_pairs_build(r->file, plan, p.get())) {
        ctx->err = "r1cs: 2^32 (wire, constraint) incidences or more";
        return K16_ERR_ARG;
    }
    r->pairs = std::move(p);
    return K16_OK;
}

// hipMalloc for the scan: out of device memory is K16_ERR_NOMEM
static int r1cs_scan_alloc(k16_ctx* ctx, void** p, size_t bytes)
{
    const hipError_t e = hipMalloc(p, std::max<size_t>(bytes, 32));
    if (e == hipSuccess) return K16_OK;
    *p       = nullptr;
    ctx->err = std::string("unbound-wire scan: hipMalloc: ") + hipGetErrorString(e);
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? K16_ERR_NOMEM : K16_ERR_HIP;
}

// list, side table and mask on the device, by the first scan
static int r1cs_scan_upload(k16_ctx* ctx, k16_r1cs* r)
{
    const R1csPairs&    P    = *r->pairs;
    const size_t        skip = P.start[1]; // wire 0's column stays on the host: see k_r1cs_incidences
    const size_t        n = P.pair.size() - skip, words = P.present.size();
    std::vector<R1csFr> side(P.side.size());
    const R1csScale     to_r9(522);
    for (size_t k = 0; k < side.size(); k++) side[k] = to_r9(P.side[k]);
    int rc;
    if ((rc = r1cs_scan_alloc(ctx, (void**)&r->d_inc, n * sizeof(R1csPair)))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, (void**)&r->d_incwire, n * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, (void**)&r->d_side, side.size() * 32))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, (void**)&r->d_bound, words * 8))) return rc;
    K16_HIP(ctx, hipHostMalloc((void**)&r->h_bound, std::max<size_t>(words * 8, 8), hipHostMallocDefault));
    hipStream_t st = ctx->stream;
    if (n) {
        K16_HIP(ctx, hipMemcpyAsync(r->d_inc, P.pair.data() + skip, n * sizeof(R1csPair), hipMemcpyHostToDevice, st));
        K16_HIP(ctx, hipMemcpyAsync(r->d_incwire, P.wire.data() + skip, n * 4, hipMemcpyHostToDevice, st));
    }
    if (!side.empty()) K16_HIP(ctx, hipMemcpyAsync(r->d_side, side.data(), side.size() * 32, hipMemcpyHostToDevice, st));
    K16_HIP(ctx, hipStreamSynchronize(st)); // (side is a local)
    r->scan_ready = true;
    return K16_OK;
}

static int r1cs_scan_run(k16_ctx* ctx, k16_r1cs* r)
{
    const R1csPairs& P     = *r->pairs;
    const uint32_t   n     = (uint32_t)P.pair.size() - P.start[1]; // all but wire 0's column
    const size_t     words = P.present.size();
    hipStream_t      st    = ctx->stream;
    K16_HIP(ctx, hipMemsetAsync(r->d_bound, 0, words * 8, st));
    if (n) {
        k16_stat_scope sc(ctx, "r1cs_incidences", st);
        hipLaunchKernelGGL(k_r1cs_incidences, dim3((unsigned)(((uint64_t)n + 255) / 256)), dim3(256), 0, st, r->d_inc, r->d_incwire, n,
                           r->d_coef, P.n_entries, r->d_side, r->d_rows, r->M, r->d_bound);
    }
    K16_HIP(ctx, hipGetLastError());
    K16_HIP(ctx, hipMemcpyAsync(r->h_bound, r->d_bound, words * 8, hipMemcpyDeviceToHost, st));
    K16_HIP(ctx, hipStreamSynchronize(st));
    return K16_OK;
}

extern "C" int k16_r1cs_unbound_wires(k16_r1cs* r, uint64_t* n_absent, uint64_t* n_unbound, uint32_t* h_wires, uint8_t* h_class,
                                      uint32_t cap, uint8_t* h_status)
{
    return k16_guard(r ? r->ctx : nullptr, [&]() -> int {
    if (!r || !n_absent || !n_unbound) return K16_ERR_ARG;
    *n_absent = *n_unbound = 0;
    k16_ctx* ctx = r->ctx;
    if (!r->have_values || r->forked_on) {
        ctx->err = "no completed check to scan";
        return K16_ERR_ARG;
    }
    int rc = r1cs_pairs_get(ctx, r);
    if (rc) return rc;
    K16_HIP(ctx, hipSetDevice(ctx->device));
    if (!r->scan_ready) rc = r1cs_scan_upload(ctx, r);
    if (!rc) rc = r1cs_scan_run(ctx, r);
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream); // nothing of the scan stays in flight
        if (!r->scan_ready) r1cs_scan_free(r);
        return rc;
    }
    const R1csPairs& P = *r->pairs;
    uint64_t         absent = 0, unbound = 0, listed = 0;
    for (size_t w = 0; w < P.present.size(); w++) {
        const uint32_t     in_word = (uint32_t)std::min<uint64_t>(64, (uint64_t)r->n_wires - 64 * (uint64_t)w);
        unsigned long long valid   = in_word == 64 ? ~0ull : (1ull << in_word) - 1;
        if (w == 0) valid &= ~1ull; // wire 0 is the constant
        const unsigned long long free_ = ~r->h_bound[w] & valid, here = P.present[w];
        absent += (uint64_t)__builtin_popcountll(free_ & ~here);
        unbound += (uint64_t)__builtin_popcountll(free_ & here);
        if (h_status)
            for (uint32_t b = 0; b < in_word; b++)
                h_status[64 * w + b] = (free_ >> b) & 1 ? ((here >> b) & 1 ? K16_WIRE_UNBOUND : K16_WIRE_ABSENT) : K16_WIRE_BOUND;
        for (unsigned long long m = free_; m && listed < cap && (h_wires || h_class); m &= m - 1, listed++) {
            const uint32_t b = (uint32_t)__builtin_ctzll(m);
            if (h_wires) h_wires[listed] = (uint32_t)(64 * w + b);
            if (h_class) h_class[listed] = (here >> b) & 1 ? K16_WIRE_UNBOUND : K16_WIRE_ABSENT;
        }
    }
    *n_absent  = absent;
    *n_unbound = unbound;
    return K16_OK;
    });
}

// ---- the second-value scan
// masks, references, list and shifts, by the first call; the incidence list itself is the unbound-wire scan's
static int r1cs_second_alloc(k16_ctx* ctx, k16_r1cs* r)
{
    const size_t words = r->pairs->present.size(), n = r->n_wires;
    int          rc;
    if ((rc = r1cs_scan_alloc(ctx, (void**)&r->d_kinds, 2 * words * 8))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, (void**)&r->d_ref, n * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, (void**)&r->d_list, n * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, (void**)&r->d_shift, n * 32))) return rc;
    K16_HIP(ctx, hipHostMalloc((void**)&r->h_kinds, std::max<size_t>(2 * words * 8, 8), hipHostMallocDefault));
    K16_HIP(ctx, hipHostMalloc((void**)&r->h_list, std::max<size_t>(n * 4, 8), hipHostMallocDefault));
    r->second_ready = true;
    return K16_OK;
}

static int r1cs_second_run(k16_ctx* ctx, k16_r1cs* r, uint64_t* n_two_valued, uint32_t* h_wires, uint8_t* h_shift, uint32_t cap,
                           uint8_t* h_status)
{
    const R1csPairs& P     = *r->pairs;
    const uint32_t   n     = (uint32_t)P.pair.size() - P.start[1]; // all but wire 0's column
    const size_t     words = P.present.size();
    const dim3       grid((unsigned)(((uint64_t)n + 255) / 256));
    hipStream_t      st = ctx->stream;
    K16_HIP(ctx, hipMemsetAsync(r->d_kinds, 0, 2 * words * 8, st));
    K16_HIP(ctx, hipMemsetAsync(r->d_ref, 0xff, (size_t)r->n_wires * 4, st));
    if (n) {
        {
            k16_stat_scope sc(ctx, "r1cs_kinds", st);
            hipLaunchKernelGGL(k_r1cs_kinds, grid, dim3(256), 0, st, r->d_inc, r->d_incwire, n, r->d_coef, P.n_entries, r->d_side,
                               r->d_rows, r->M, r->d_kinds, r->d_kinds + words, r->d_ref);
        }
        {
            k16_stat_scope sc(ctx, "r1cs_agree", st);
            hipLaunchKernelGGL(k_r1cs_agree, grid, dim3(256), 0, st, r->d_inc, r->d_incwire, n, r->d_coef, P.n_entries, r->d_side,
                               r->d_rows, r->M, r->d_ref, r->d_kinds);
        }
    }
    K16_HIP(ctx, hipGetLastError());
    K16_HIP(ctx, hipMemcpyAsync(r->h_kinds, r->d_kinds, 2 * words * 8, hipMemcpyDeviceToHost, st));
    K16_HIP(ctx, hipStreamSynchronize(st));
    const unsigned long long *pinned = r->h_kinds, *rooted = r->h_kinds + words;
    const bool                want_list = (h_wires || h_shift) && cap;
    uint64_t                  count = 0;
    uint32_t                  listed = 0;
    for (size_t w = 0; w < words; w++) {
        const uint32_t     in_word = (uint32_t)std::min<uint64_t>(64, (uint64_t)r->n_wires - 64 * (uint64_t)w);
        unsigned long long valid   = in_word == 64 ? ~0ull : (1ull << in_word) - 1;
        if (w == 0) valid &= ~1ull; // wire 0 is the constant
        // bound as k_r1cs_incidences finds it: lin != 0 or quad != 0 somewhere, a PIN or a ROOT (a clash is among ROOTs)
        const unsigned long long free_ = ~(pinned[w] | rooted[w]) & valid, here = P.present[w], two = rooted[w] & ~pinned[w] & valid;
        count += (uint64_t)__builtin_popcountll(two);
        if (h_status)
            for (uint32_t b = 0; b < in_word; b++)
                h_status[64 * w + b] = (two >> b) & 1    ? K16_WIRE_TWO_VALUED
                                       : (free_ >> b) & 1 ? ((here >> b) & 1 ? K16_WIRE_UNBOUND : K16_WIRE_ABSENT)
                                                          : K16_WIRE_BOUND;
        for (unsigned long long m = two; m && listed < cap && want_list; m &= m - 1) r->h_list[listed++] = (uint32_t)(64 * w + (uint32_t)__builtin_ctzll(m));
    }
    *n_two_valued = count;
    if (h_wires && listed) memcpy(h_wires, r->h_list, (size_t)listed * 4);
    if (h_shift && listed) {
        K16_HIP(ctx, hipMemcpyAsync(r->d_list, r->h_list, (size_t)listed * 4, hipMemcpyHostToDevice, st));
        {
            k16_stat_scope sc(ctx, "r1cs_shifts", st);
            hipLaunchKernelGGL(k_r1cs_shifts, dim3((listed + 63) / 64), dim3(64), 0, st, r->d_list, listed, r->d_inc, n, r->d_coef,
                               P.n_entries, r->d_side, r->d_rows, r->M, r->d_ref, r->d_shift);
        }
        K16_HIP(ctx, hipGetLastError());
        K16_HIP(ctx, hipMemcpyAsync(h_shift, r->d_shift, (size_t)listed * 32, hipMemcpyDeviceToHost, st));
        K16_HIP(ctx, hipStreamSynchronize(st));
    }
    return K16_OK;
}

extern "C" int k16_r1cs_second_values(k16_r1cs* r, uint64_t* n_two_valued, uint32_t* h_wires, uint8_t* h_shift, uint32_t cap,
                                      uint8_t* h_status)
{
    return k16_guard(r ? r->ctx : nullptr, [&]() -> int {
    if (!r || !n_two_valued) return K16_ERR_ARG;
    *n_two_valued = 0;
    k16_ctx* ctx  = r->ctx;
    if (!r->have_values || r->forked_on) {
        ctx->err = "no completed check to scan";
        return K16_ERR_ARG;
    }
    int rc = r1cs_pairs_get(ctx, r);
    if (rc) return rc;
    K16_HIP(ctx, hipSetDevice(ctx->device));
    if (!r->scan_ready) rc = r1cs_scan_upload(ctx, r);
    if (!rc && !r->second_ready) rc = r1cs_second_alloc(ctx, r);
    if (!rc) rc = r1cs_second_run(ctx, r, n_two_valued, h_wires, h_shift, cap, h_status);
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream); // nothing of the scan stays in flight
        if (!r->second_ready) r1cs_second_free(r);
        if (!r->scan_ready) r1cs_scan_free(r);
        *n_two_valued = 0;
        return rc;
    }
    return K16_OK;
    });
}

// ---- the determinism closure
// column starts, masks, the two words per constraint, the maps and the two lists, by the first call
static int r1cs_det_alloc(k16_ctx* ctx, k16_r1cs* r)
{
    const R1csPairs& P     = *r->pairs;
    const size_t     words = P.present.size(), n = r->n_wires, M = r->M;
    int              rc;
    if ((rc = r1cs_scan_alloc(ctx, (void**)&r->d_det_start, (n + 1) * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, (void**)&r->d_det_masks, 2 * words * 8))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, (void**)&r->d_det_cnt, 2 * M * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, (void**)&r->d_det_by, 2 * n * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, (void**)&r->d_det_cand, M * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, (void**)&r->d_det_front, n * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, (void**)&r->d_det_state, sizeof(DetState)))) return rc;
    K16_HIP(ctx, hipHostMalloc((void**)&r->h_det_masks, std::max<size_t>(2 * words * 8, 8), hipHostMallocDefault));
    K16_HIP(ctx, hipHostMalloc((void**)&r->h_det_rec, sizeof(DetRecord), hipHostMallocMapped | hipHostMallocCoherent));
    K16_HIP(ctx, hipHostGetDevicePointer((void**)&r->d_det_rec, r->h_det_rec, 0));
    // the device list leaves wire 0's column out: its columns start that much lower
    const uint32_t        skip = P.start[1];
    std::vector<uint32_t> start(n + 1);
    for (size_t i = 0; i <= n; i++) start[i] = std::max(P.start[i], skip) - skip;
    K16_HIP(ctx, hipMemcpyAsync(r->d_det_start, start.data(), (n + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    K16_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (start is a local)
    r->det_ready = true;
    return K16_OK;
}

// h_det_masks[0 .. words) holds the seed.  Leaves `known` in h_det_masks[words ..) and the maps on the device.
static int r1cs_det_run(k16_ctx* ctx, k16_r1cs* r, uint32_t* n_rounds)
{
    const R1csPairs& P     = *r->pairs;
    const uint32_t   n     = (uint32_t)P.pair.size() - P.start[1]; // all but wire 0's column
    const size_t     words = P.present.size();
    const uint32_t   M = r->M, n_wires = r->n_wires;
    hipStream_t      st = ctx->stream;
    unsigned long long *d_seed = r->d_det_masks, *d_known = r->d_det_masks + words;
    uint32_t *          d_cnt = r->d_det_cnt, *d_xr = r->d_det_cnt + M, *d_by = r->d_det_by, *d_round = r->d_det_by + n_wires;
    auto blocks = [](uint64_t lanes) { return dim3((unsigned)((lanes + 255) / 256)); };
    auto capped = [](uint64_t lanes) { return dim3((unsigned)std::min<uint64_t>((lanes + 255) / 256, DET_GRID)); };
    *n_rounds   = 0;
    r->h_det_rec->n_front = r->h_det_rec->n_cand = 0;
    K16_HIP(ctx, hipMemcpyAsync(d_seed, r->h_det_masks, words * 8, hipMemcpyHostToDevice, st));
    K16_HIP(ctx, hipMemcpyAsync(d_known, r->h_det_masks, words * 8, hipMemcpyHostToDevice, st));
    K16_HIP(ctx, hipMemsetAsync(r->d_det_by, 0xff, 2 * (size_t)n_wires * 4, st));
    K16_HIP(ctx, hipMemsetAsync(r->d_det_state, 0, sizeof(DetState), st));
    if (n && M) {
        K16_HIP(ctx, hipMemsetAsync(r->d_det_cnt, 0, 2 * (size_t)M * 4, st));
        {
            k16_stat_scope sc(ctx, "r1cs_det_init", st);
            hipLaunchKernelGGL(k_r1cs_det_init, blocks(n), dim3(256), 0, st, r->d_inc, r->d_incwire, n, n_wires, M, d_seed, d_cnt, d_xr);
            hipLaunchKernelGGL(k_r1cs_det_first, capped(M), dim3(256), 0, st, d_cnt, M, r->d_det_cand, r->d_det_state, r->d_det_rec);
        }
        K16_HIP(ctx, hipGetLastError());
    }
    K16_HIP(ctx, hipStreamSynchronize(st));
    // round k judges the candidates [c0, c1) and derives the frontier [f0, f1)
    uint32_t c0 = 0, c1 = r->h_det_rec->n_cand, f0 = 0, round = 0;
    while (c1 > c0) {
        // every round that goes on adds a wire, and wire 0 is never added: at most n_wires - 1 rounds
        if (round + 1 >= n_wires || c1 > M) {
            ctx->err = "determinism closure: more rounds than wires";
            return K16_ERR_HIP;
        }
        round++;
        {
            k16_stat_scope sc(ctx, "r1cs_det_derive", st);
            hipLaunchKernelGGL(k_r1cs_det_derive, blocks(c1 - c0), dim3(256), 0, st, r->d_det_cand + c0, c1 - c0, r->d_inc,
                               r->d_incwire, n, r->d_coef, P.n_entries, r->d_side, r->d_rows, M, r->d_mask, d_known, d_cnt, d_xr,
                               n_wires, d_by, r->d_det_front, r->d_det_state);
        }
        {
            // a candidate derives one wire at the most: the frontier is no longer than the candidates' range
            k16_stat_scope sc(ctx, "r1cs_det_expand", st);
            hipLaunchKernelGGL(k_r1cs_det_expand, capped(c1 - c0), dim3(256), 0, st, r->d_det_front, f0, round, r->d_det_start,
                               r->d_inc, n, n_wires, M, d_known, d_round, d_cnt, d_xr, r->d_det_cand, r->d_det_state, r->d_det_rec);
        }
        K16_HIP(ctx, hipGetLastError());
        K16_HIP(ctx, hipStreamSynchronize(st));
        const uint32_t f1 = r->h_det_rec->n_front, c2 = r->h_det_rec->n_cand;
        if (f1 < f0 || f1 > n_wires || c2 < c1) {
            ctx->err = "determinism closure: a list shrank or outgrew its room";
            return K16_ERR_HIP;
        }
        if (f1 == f0) { // nothing derived: the level before was the fixed point
            round--;
            break;
        }
        f0 = f1, c0 = c1, c1 = c2;
    }
    *n_rounds = round;
    K16_HIP(ctx, hipMemcpyAsync(r->h_det_masks + words, d_known, words * 8, hipMemcpyDeviceToHost, st));
    K16_HIP(ctx, hipStreamSynchronize(st));
    return K16_OK;
}

// round and by as the device left them (the caller writes round 0 for the seed), only when asked for
static int r1cs_det_maps(k16_ctx* ctx, k16_r1cs* r, uint32_t* h_round, uint32_t* h_by)
{
    const size_t bytes = (size_t)r->n_wires * 4;
    if (h_by) K16_HIP(ctx, hipMemcpyAsync(h_by, r->d_det_by, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (h_round) K16_HIP(ctx, hipMemcpyAsync(h_round, r->d_det_by + r->n_wires, bytes, hipMemcpyDeviceToHost, ctx->stream));
    K16_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return K16_OK;
}

extern "C" int k16_r1cs_determined_wires(k16_r1cs* r, const uint32_t* h_seed, uint32_t n_seed, uint64_t* n_derived, uint64_t* n_absent,
                                         uint64_t* n_open, uint32_t* n_rounds, uint32_t* h_wires, uint32_t cap, uint8_t* h_status,
                                         uint32_t* h_round, uint32_t* h_by)
{
    return k16_guard(r ? r->ctx : nullptr, [&]() -> int {
    if (!r || !n_derived || !n_absent || !n_open || !n_rounds || (!h_seed && n_seed)) return K16_ERR_ARG;
    *n_derived = *n_absent = *n_open = 0;
    *n_rounds                        = 0;
    k16_ctx* ctx                     = r->ctx;
    if (!r->have_values || r->forked_on) {
        ctx->err = "no completed check to scan";
        return K16_ERR_ARG;
    }
    // the default seed: what the file's header calls inputs, in the iden3 wire order 1 | public outputs | public inputs | private inputs
    const uint64_t in0 = (uint64_t)r->file.n_pub_out + 1, in1 = in0 + r->file.n_pub_in + r->file.n_prv_in;
    if (!h_seed && in1 > r->n_wires) {
        ctx->err = "the header's input wires reach beyond nWires";
        return K16_ERR_ARG;
    }
    for (uint32_t k = 0; k < n_seed; k++)
        if (h_seed[k] >= r->n_wires) {
            ctx->err = "seed wire number out of range";
            return K16_ERR_ARG;
        }
    int rc = r1cs_pairs_get(ctx, r);
    if (rc) return rc;
    K16_HIP(ctx, hipSetDevice(ctx->device));
    if (!r->scan_ready) rc = r1cs_scan_upload(ctx, r);
    if (!rc && !r->det_ready) rc = r1cs_det_alloc(ctx, r);
    const size_t        words = r->pairs->present.size();
    unsigned long long* seed  = r->h_det_masks;
    if (!rc) {
        memset(seed, 0, words * 8);
        seed[0] = 1ull; // wire 0
        if (h_seed)
            for (uint32_t k = 0; k < n_seed; k++) seed[h_seed[k] >> 6] |= 1ull << (h_seed[k] & 63u);
        else
            for (uint64_t i = in0; i < in1; i++) seed[i >> 6] |= 1ull << (i & 63u);
        rc = r1cs_det_run(ctx, r, n_rounds);
    }
    if (!rc && (h_round || h_by)) rc = r1cs_det_maps(ctx, r, h_round, h_by);
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream); // nothing of the scan stays in flight
        if (!r->det_ready) r1cs_det_free(r);
        if (!r->scan_ready) r1cs_scan_free(r);
        *n_rounds = 0;
        return rc;
    }
    const R1csPairs&          P     = *r->pairs;
    const unsigned long long* known = r->h_det_masks + words;
    uint64_t                  derived = 0, absent = 0, open = 0, listed = 0;
    for (size_t w = 0; w < words; w++) {
        const uint32_t           in_word = (uint32_t)std::min<uint64_t>(64, (uint64_t)r->n_wires - 64 * (uint64_t)w);
        const unsigned long long valid = in_word == 64 ? ~0ull : (1ull << in_word) - 1, here = P.present[w];
        const unsigned long long out = ~known[w] & valid, got = known[w] & ~seed[w] & valid;
        derived += (uint64_t)__builtin_popcountll(got);
        absent += (uint64_t)__builtin_popcountll(out & ~here);
        open += (uint64_t)__builtin_popcountll(out & here);
        if (h_status)
            for (uint32_t b = 0; b < in_word; b++)
                h_status[64 * w + b] = (seed[w] >> b) & 1   ? K16_DET_SEED
                                       : (got >> b) & 1     ? K16_DET_DERIVED
                                       : (here >> b) & 1    ? K16_DET_OPEN
                                                            : K16_DET_ABSENT;
        if (h_round)
            for (unsigned long long m = seed[w] & valid; m; m &= m - 1) h_round[64 * w + (uint32_t)__builtin_ctzll(m)] = 0;
        for (unsigned long long m = out & here; m && listed < cap && h_wires; m &= m - 1) h_wires[listed++] = (uint32_t)(64 * w + (uint32_t)__builtin_ctzll(m));
    }
    *n_derived = derived, *n_absent = absent, *n_open = open;
    return K16_OK;
    });
}

extern "C" int k16_r1cs_wire_constraints(k16_r1cs* r, uint32_t wire, uint64_t* n, uint32_t* h_constraints, uint32_t cap)
{
    return k16_guard(r ? r->ctx : nullptr, [&]() -> int {
    if (!r || !n) return K16_ERR_ARG;
    *n = 0;
    if (wire >= r->n_wires) {
        r->ctx->err = "wire number out of range";
        return K16_ERR_ARG;
    }
    const int rc = r1cs_pairs_get(r->ctx, r);
    if (rc) return rc;
    const R1csPairs& P = *r->pairs;
    *n                 = P.start[wire + 1] - P.start[wire];
    const uint64_t k_n = std::min<uint64_t>(*n, cap);
    for (uint64_t k = 0; h_constraints && k < k_n; k++) h_constraints[k] = P.pair[P.start[wire] + k].constraint;
    return K16_OK;
    });
}

extern "C" int k16_r1cs_incidences(k16_r1cs* r, uint64_t* n_pairs)
{
    return k16_guard(r ? r->ctx : nullptr, [&]() -> int {
    if (!r || !n_pairs) return K16_ERR_ARG;
    *n_pairs     = 0;
    const int rc = r1cs_pairs_get(r->ctx, r);
    if (rc) return rc;
    *n_pairs = r->pairs->n_pairs();
    return K16_OK;
    });
}

extern "C" int k16_r1cs_match_zkey(k16_ctx* ctx, const k16_r1cs* r, const void* zkey, size_t size, uint32_t* mismatch)
{
    return k16_guard(ctx, [&]() -> int {
    if (!ctx || !r || !zkey || !mismatch) return K16_ERR_ARG;
    *mismatch = 0;
    R1csMismatch mm;
    const char*  why = "";
    const int    rc  = r1cs_match_zkey(r->file, (const uint8_t*)zkey, size, &mm, &why);
    if (rc) {
        ctx->err = *why ? why : "zkey: malformed header or coefficient section";
        return rc;
    }
    *mismatch = mm.kind;
    if (mm.kind) {
        static const char* const kinds[] = {"", "header", "matrix A", "matrix B", "public rows"};
        char                     buf[256];
        snprintf(buf, sizeof buf, "r1cs / zkey mismatch: %s, constraint %u, wire %u (%s)", kinds[mm.kind], mm.constraint, mm.wire, why);
        ctx->err = buf;
    }
    return K16_OK;
    });
}
