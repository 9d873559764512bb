// r1cs_scan.hip -- the diagnostics on top of the R1CS witness check (include/k16.h; r1cs_check.hip makes what they read): three
// questions about the sums a completed check left in d_rows, all answered by walks over ONE list, the (wire, constraint)
// incidences of the circuit (r1cs_pairs.h), ordered by wire.
//   k16_r1cs_unbound_wires     which wires could take any value without moving a residual?  k_r1cs_incidences
//   k16_r1cs_second_values     which admit exactly ONE other value, every other wire held fixed?  k_r1cs_kinds, _agree, _shifts (10c)
//   k16_r1cs_determined_wires  which does the circuit force, given the seed wires?  k_r1cs_det_init, _first, _derive, _expand (10d)
//   k16_r1cs_complete_witness  which VALUES do the given wires force?  the closure's frontier + k_r1cs_solve_mask, _derive, _commit, _close (10e)
//   k16_r1cs_complete_witness_ex  ... and which bit decompositions?  k_r1cs_bits_filter, k_r1cs_solve_bits, k_r1cs_bits_commit over the
//                              boolean marks of k16_r1cs_boolean_wires (r1cs_bools.h) (10f)
//   k16_r1cs_determined_wires_ex  ... and which wires do the bit decompositions force?  k_r1cs_held, k_r1cs_bits_filter,
//                              k_r1cs_det_bits over the marking rows the check left unbroken (k16_r1cs_held_wires) (10g)
// Each kernel is described where it stands.  The list and every buffer here are made by the first call that needs them: create
// and check calls allocate and launch nothing of this file.  From masks to counts, lists and status bytes: r1cs_masks.h.
#include <string.h>
#include <memory>
#include <string>
#include <vector>
#include "r1cs_obj.h"
#include "frinv_dev.h"
#include "r1cs_bools.h"
#include "r1cs_masks.h"
#include "r1cs_open.h"
#include "r1cs_pairs.h"
#include "r1cs_rows.h"
#include "spmv_dev.h"

using namespace k16;

static_assert(sizeof(R1csPair) == sizeof(uint4), "an incidence is one 16-byte load");
static_assert(sizeof(R1csRowRef) == sizeof(uint2), "a term of the row view is one 8-byte load");

namespace {

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

// The terms of an incidence.  Change wire i alone by d: the residual a_c b_c - c_c of constraint c moves by d lin + d^2 quad with
//   lin = A^ b_c + B^ a_c - C^,  quad = A^ B^      (A^, B^, C^: the merged coefficients of wire i in constraint c)
// quad: r is prime, so a product of two non-zero residues is non-zero, and r1cs_pairs.h names a coefficient only when its merged
// sum is non-zero: quad != 0 exactly when the incidence names both A^ and B^.  Whether it is zero needs no product.
// Scalings: a coefficient k is stored as k * 2^522 mod r (coef, and side in the same scaling), a sum s lies in rows as the R'
// value s * 2^261; frmul9 divides by 2^261.  Bounds: coefficients < r, sums < 2r (+ 2^-17 r): every product below is < 2r.
//   lin   frmul9(A^ 2^522, b 2^261) + frmul9(B^ 2^522, a 2^261) - C^ 2^522  =  lin 2^522: the products and the bare C^ term carry
//         the SAME factor.  Where one of A^, B^ is absent, lin is ONE product (or none) minus C^; where both are there, fradd9 of
//         two values < 2r (its bound is < 4r); then frsub9 with the subtrahend C^ 2^522 < r (its bound is < 2r).  fr9_nonzero
//         divides by 2^261 once more and looks at the canonical representative of lin * 2^261: zero exactly when r divides lin
//         (the operands are lazy representatives below 2r, as in k_r1cs_judge)
//   quad  frmul9(A^ 2^522, B^ 2^522) = quad 2^783; coefficients < r: the product is < 2r.  The kind of an incidence does not
//         need it, the comparison and the shift do
//   two ROOTs (lin, quad), (lin0, quad0) give the same d exactly when lin quad0 = lin0 quad (quad, quad0 != 0):
//         frmul9(lin 2^522, quad0 2^783) and frmul9(lin0 2^522, quad 2^783) both carry 2^1044; operands < 2r, products < 2r, and
//         the difference goes through fr9_nonzero: products of coefficients like r - 1 agree only modulo r
//   d     frmul9(quad 2^783, 1) = quad 2^522 = (quad 2^261) 2^261, the R' value of quad 2^261; frinv9 returns the R' value of
//         its inverse, quad^-1 2^-261 2^261 = quad^-1 with factor 1; frmul9(lin 2^522, quad^-1) = (lin / quad) 2^261, an R' value
//         again, negated by frsub9(0, .) -- and fr9_to_standard divides by 2^261: the canonical -lin / quad.
//
// The device list as every kernel sees it, one kernel argument.  inc / wire: n_pairs incidences ordered by wire and, within a
// wire, by constraint (the host leaves wire 0's column out, see k_r1cs_incidences); inc[i].x: the constraint, .y / .z / .w: the
// positions of A^ / B^ / C^.  Positions: < n_entries -> coef, n_entries + k -> side[k], R1CS_PAIR_NONE -> 0.  rows: A.w | B.w |
// C.w of the last completed check, M packed R' values each.
struct IncList {
    const uint4* __restrict__ inc;
    const uint32_t* __restrict__ wire;
    uint32_t n_pairs;
    const Fr* __restrict__ coef;
    uint32_t n_entries;
    const Fr* __restrict__ side;
    const Fr* __restrict__ rows;
    uint32_t M;
    __device__ __forceinline__ Fr9 at(uint32_t p) const { return ld_r9(p < n_entries ? &coef[p] : &side[p - n_entries]); }
};
struct IncTerms {
    Fr9  lin;
    bool has_quad; // both A^ and B^ are there: quad != 0
};
// lin 2^522 of incidence e
__device__ __forceinline__ IncTerms inc_terms(const uint4 e, const IncList& L)
{
    const bool a = e.y != R1CS_PAIR_NONE, b = e.z != R1CS_PAIR_NONE;
    IncTerms   t;
    t.lin      = fq9_zero();
    t.has_quad = a && b;
    if (a || b) { // B^ a_c where B^ is there, else A^ b_c: the one product, or the second of two
        t.lin = frmul9(L.at(b ? e.z : e.y), ld_r9(&L.rows[b ? e.x : (size_t)L.M + e.x]));
        if (t.has_quad) t.lin = fradd9(frmul9(L.at(e.y), ld_r9(&L.rows[(size_t)L.M + e.x])), t.lin);
    }
    if (e.w != R1CS_PAIR_NONE) t.lin = frsub9(t.lin, L.at(e.w));
    return t;
}
// quad 2^783 of an incidence that names both
__device__ __forceinline__ Fr9 inc_quad(const uint4 e, const IncList& L) { return frmul9(L.at(e.y), L.at(e.z)); }

// The unbound-wire scan: a wire is bound by constraint c when lin != 0 or quad != 0 (mod r).  An incidence that names both A^
// and B^ is bound without any product.
// bound: ceil(n_wires / 64) words, cleared before the launch, bit i = wire i is bound.  The list is ordered by wire, so the
// lanes of a wave whose wires share a mask word are neighbours: their bits are ORed over the wave first and ONE lane per word
// issues the atomicOr, and only where the word does not show the bits yet (atomics on ONE address queue up behind each other
// across the whole device: a wire that sits in a large part of the constraints would cost one per wave); an OR gives the same
// mask whatever order the lanes run in.  Wire 0, the constant, is BOUND by definition: the host leaves its column -- the
// longest of a real circuit -- out of the launch.  Launched with whole waves.
__global__ void __launch_bounds__(256) k_r1cs_incidences(const IncList L, unsigned long long* bound)
{
    const uint32_t i   = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t       w   = 0xffffffffu; // (no wire: the lanes behind the list)
    bool           hit = false;
    if (i < L.n_pairs) {
        const uint4 e = L.inc[i];
        w             = L.wire[i];
        hit           = (e.y != R1CS_PAIR_NONE && e.z != R1CS_PAIR_NONE) || fr9_nonzero(inc_terms(e, L).lin);
    }
    wave_or_into(bound, w >> 6, hit ? 1ull << (w & 63u) : 0ull);
}

// The second-value scan.  An incidence is FREE (lin = quad = 0: every d leaves the residual), a PIN
// (exactly one of them is zero: no d != 0 leaves it -- d lin = 0 or d^2 quad = 0 has the root 0 alone, r being prime) or a ROOT
// (neither is zero: d lin + d^2 quad = 0 has exactly one other root, d = -lin / quad).  A wire is TWO-VALUED when it has no PIN,
// at least one ROOT, and all its ROOTs give the same d.
// pinned / rooted: ceil(n_wires / 64) words each, cleared before the launch: bit i = wire i has a PIN / a ROOT incidence,
// merged per word and wave as in k_r1cs_incidences.  ref[n_wires], all ones before the launch: the lowest ROOT incidence of each
// wire.  The list is ordered by wire and, within a wire, ascending: among the lanes of a wave that share a wire the FIRST ROOT
// lane holds the wave's minimum, it alone issues the atomicMin, and only where ref does not show an index that low yet (ref only
// ever falls: a read that lags behind costs an atomic for nothing).  One atomic per wire and wave at the most, however long the
// column; a minimum is the same whatever order the lanes run in.  Launched with whole waves.
__global__ void __launch_bounds__(256) k_r1cs_kinds(const IncList L, unsigned long long* pinned, unsigned long long* rooted, uint32_t* ref)
{
    const uint32_t i   = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t       w   = 0xffffffffu; // (no wire: the lanes behind the list)
    bool           pin = false, root = false;
    if (i < L.n_pairs) {
        w                 = L.wire[i];
        const IncTerms t  = inc_terms(L.inc[i], L);
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
__global__ void __launch_bounds__(256) k_r1cs_agree(const IncList L, const uint32_t* __restrict__ ref, unsigned long long* pinned)
{
    const uint32_t i     = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t       w     = 0xffffffffu;
    bool           clash = false;
    if (i < L.n_pairs) {
        w             = L.wire[i];
        const uint4 e = L.inc[i];
        const uint32_t j = ref[w];
        if (e.y != R1CS_PAIR_NONE && e.z != R1CS_PAIR_NONE && j != i && j < L.n_pairs) {
            const IncTerms t = inc_terms(e, L);
            if (fr9_nonzero(t.lin)) {
                const uint4    e0 = L.inc[j];
                const IncTerms t0 = inc_terms(e0, L);
                clash = fr9_nonzero(frsub9(frmul9(t.lin, inc_quad(e0, L)), frmul9(t0.lin, inc_quad(e, L))));
            }
        }
    }
    wave_or_into(pinned, w >> 6, clash ? 1ull << (w & 63u) : 0ull);
}

// list[n]: two-valued wires; shift[k] = -lin0 / quad0 of list[k]'s reference incidence, standard form (canonical; non-zero, as
// lin0 != 0).  One inversion per lane: the work is the list's, not the circuit's.
__global__ void __launch_bounds__(64) k_r1cs_shifts(const uint32_t* __restrict__ list, uint32_t n, const IncList L,
                                                    const uint32_t* __restrict__ ref, Fr* __restrict__ shift)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t j = ref[list[k]];
    if (j >= L.n_pairs) return; // (a listed wire has a ROOT incidence)
    const uint4    e0 = L.inc[j];
    const IncTerms t0 = inc_terms(e0, L);
    Fr9            one = fq9_zero();
    one.l[0]           = 1;
    const Fr9 qinv = frinv9(frmul9(inc_quad(e0, L), one));
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
__global__ void __launch_bounds__(256) k_r1cs_det_init(const IncList L, uint32_t n_wires, const unsigned long long* __restrict__ seed,
                                                       uint32_t* cnt, uint32_t* xr)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.n_pairs) return;
    const uint32_t w = L.wire[i], c = L.inc[i].x;
    if (w >= n_wires || c >= L.M || det_bit(seed, w)) return;
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
__global__ void __launch_bounds__(256) k_r1cs_det_derive(const uint32_t* __restrict__ cand, uint32_t n, const IncList L,
                                                         const unsigned long long* __restrict__ verdict, const unsigned long long* __restrict__ known,
                                                         const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ xr, uint32_t n_wires, uint32_t* by,
                                                         uint32_t* __restrict__ front, DetState* st)
{
    const uint32_t k   = blockIdx.x * blockDim.x + threadIdx.x;
    bool           add = false;
    uint32_t       x   = 0;
    if (k < n) {
        const uint32_t c = cand[k];
        if (c < L.M && !det_bit(verdict, c) && cnt[c] == 1u) {
            const uint32_t idx = xr[c];
            if (idx < L.n_pairs) {
                x = L.wire[idx];
                if (x < n_wires && !det_bit(known, x)) {
                    const IncTerms t = inc_terms(L.inc[idx], L);
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
                                                         const uint32_t* __restrict__ start, const IncList L, uint32_t n_wires,
                                                         unsigned long long* known, uint32_t* __restrict__ round_of, uint32_t* cnt, uint32_t* xr,
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
                e           = min(start[x + 1], L.n_pairs);
            }
        }
        wave_or_into(known, x >> 6, x != DET_NONE ? 1ull << (x & 63u) : 0ull);
        // one incidence: leaves the outside count of its constraint
        auto leave = [&](bool act, uint32_t idx) {
            bool     listed = false;
            uint32_t c      = 0;
            if (act) {
                c = L.inc[idx].x;
                if (c < L.M) {
                    listed = atomicSub(&cnt[c], 1u) == 2u;
                    atomicXor(&xr[c], idx);
                }
            }
            wave_append(cand, &st->n_cand, L.M, listed, c);
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

// The witness completion (k16_r1cs_complete_witness): the closure's frontier with VALUES.  K_0 holds the
// given wires; with respect to K_k a constraint c with exactly ONE incidence (x, c) outside is a polynomial in x,
//     quad x^2 + lin x + k0,   quad = A^ B^,  lin = A^ b0 + B^ a0 - C^,  k0 = a0 b0 - c0
// a0, b0, c0 being the sums of c's three rows over its wires in K_k; quad = 0 and lin != 0 give x = -k0 / lin, anything else
// gives nothing.  cnt, xr, the two lists, the record and the kernels k_r1cs_det_init, _first and _expand are the closure's.
// INVARIANT: a wire outside K holds 0 in wtns.  A plain sum over a row IS the sum over its wires in K, x's own terms add
// nothing, and a wire whose coefficients cancel inside a row needs no special case.
//   k_r1cs_solve_mask    one lane per wire: outside the givens -> 0 (whatever the caller had there), a given value >= r or
//                        wire 0 != 1 -> the flag word: the host reads it before the first round
//   k_r1cs_solve_derive  one lane per candidate of this round: cnt still 1, the outside incidence names not both A^ and B^
//                        (quad != 0 otherwise, see inc_terms: no product needed), three row sums through the row view, lin != 0
//                        -> the value into val[c], atomicMin(by[x], c), the first claim appends x to the frontier
//   k_r1cs_solve_commit  one lane per frontier wire of this round: wtns[x] = val[by[x]]
//   k_r1cs_det_expand    as in the closure
//   k_r1cs_solve_close   after the fixed point and the check's own kernels on wtns: one lane per constraint, cnt != 0 -> open;
//                        the verdicts of the open constraints are taken out
// THE COMMIT HAZARD: two candidates of one round may claim the same x with different values (then no witness agrees with the
// givens).  by[x] is a minimum and ends the same in every launch order; a value stored by the claiming lane would be the LAST
// claimer's, not the lowest's.  So a candidate keeps its value in a slot of its own -- val[c]: a constraint is a candidate once
// -- and wtns[x] is written by the next kernel, when by[x] is final.  wtns is only read in k_r1cs_solve_derive, and 0 is a value
// like any other: what is known is the `known` mask's to say, never the value's.
// Scalings (see inc_terms): a coefficient k lies in coef / side as k 2^522, a wire's value v in wtns in standard form, v < r.
//   term  frmul9(k 2^522, v) = k v 2^261, the R' value of the product, < 2r; fradd9 keeps a sum < 2r: a0, b0, c0 are R' values,
//         exactly what k_r1cs_rows leaves in d_rows
//   lin   frmul9(A^ 2^522, b0 2^261) = A^ b0 2^522 (or B^ a0; never both: quad = 0), frsub9 with C^ 2^522 < r: lin 2^522,
//         the value inc_terms forms, on these sums.  fr9_nonzero: zero exactly when r divides lin
//   k0    frmul9(a0 2^261, b0 2^261) = a0 b0 2^261, frsub9 with c0 2^261 < 2r: k0 2^261, an R' value
//   x     frmul9(lin 2^522, 1) = lin 2^261, the R' value of lin; frinv9 returns the R' value of its inverse, lin^-1 2^261;
//         frmul9(k0 2^261, lin^-1 2^261) = (k0 / lin) 2^261, negated by frsub9(0, .) and brought to the canonical standard form
//         by fr9_to_standard: the bytes that go into wtns and back to the caller.
constexpr uint32_t SOLVE_SHORT = 16; // terms in the three rows of a candidate up to which its lane walks them alone

// The device row view (r1cs_rows.h): start[3 M + 1], term[t].x the wire, .y the position of the coefficient in coef.
struct RowView {
    const uint32_t* __restrict__ start;
    const uint2* __restrict__ term;
};
__device__ __forceinline__ Fr9 solve_term(const RowView& V, const IncList& L, const Fr* __restrict__ wtns, uint32_t n_wires, uint32_t t)
{
    const uint2 e = V.term[t];
    if (e.x >= n_wires || e.y >= L.n_entries) return fq9_zero();
    return frmul9(ld_r9(&L.coef[e.y]), ld_r9(&wtns[e.x]));
}

// given: ceil(n_wires / 64) words; flags: one word, cleared before the launch (WTNS_*, as k_r1cs_wtns sets them)
__global__ void __launch_bounds__(256) k_r1cs_solve_mask(uint4* __restrict__ wtns, uint32_t n_wires, const unsigned long long* __restrict__ given,
                                                         unsigned long long* __restrict__ flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_wires) return;
    if (!det_bit(given, i)) {
        wtns[2 * (size_t)i] = wtns[2 * (size_t)i + 1] = make_uint4(0, 0, 0, 0);
        return;
    }
    const uint4        lo = wtns[2 * (size_t)i], hi = wtns[2 * (size_t)i + 1];
    const uint32_t     v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    unsigned long long bad  = 0;
    bool               geq  = true; // v >= r?
    for (int k = 7; k >= 0; k--) {
        if (v[k] != FrParams::P[k]) {
            geq = v[k] > FrParams::P[k];
            break;
        }
    }
    if (geq) bad |= WTNS_NOT_BELOW_R;
    if (i == 0 && (v[0] != 1u || (v[1] | v[2] | v[3] | v[4] | v[5] | v[6] | v[7]) != 0)) bad |= WTNS_WIRE0_NOT_ONE;
    if (bad) atomicOr(flags, bad);
}

// cand[0 .. n): the candidates of this round.  val: M slots.  Launched with whole waves.
__global__ void __launch_bounds__(256) k_r1cs_solve_derive(const uint32_t* __restrict__ cand, uint32_t n, const IncList L, const RowView V,
                                                           const Fr* __restrict__ wtns, const unsigned long long* __restrict__ known,
                                                           const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ xr, uint32_t n_wires,
                                                           uint32_t* by, Fr* __restrict__ val, uint32_t* __restrict__ front, DetState* st)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
    bool           live = false;
    uint32_t       c = 0, x = 0;
    uint4          e = make_uint4(0, R1CS_PAIR_NONE, R1CS_PAIR_NONE, R1CS_PAIR_NONE);
    if (k < n) {
        c = cand[k];
        if (c < L.M && cnt[c] == 1u) { // (a constraint may have fallen on to 0 in the expansion that listed it)
            const uint32_t idx = xr[c];
            if (idx < L.n_pairs) {
                x    = L.wire[idx];
                e    = L.inc[idx];
                live = x < n_wires && e.x == c && !det_bit(known, x) && !(e.y != R1CS_PAIR_NONE && e.z != R1CS_PAIR_NONE);
            }
        }
    }
    // the three row sums: a short candidate by its lane, a long one by the whole wave, 64 terms a step
    uint32_t s[3] = {0, 0, 0}, len[3] = {0, 0, 0};
    Fr9      sum[3] = {fq9_zero(), fq9_zero(), fq9_zero()};
    if (live) {
#pragma unroll
        for (int m = 0; m < 3; m++) {
            s[m]               = V.start[(size_t)m * L.M + c];
            const uint32_t end = V.start[(size_t)m * L.M + c + 1];
            len[m]             = end > s[m] ? end - s[m] : 0;
        }
    }
    const uint32_t total = len[0] + len[1] + len[2];
    if (live && total <= SOLVE_SHORT) {
#pragma unroll
        for (int m = 0; m < 3; m++)
            for (uint32_t t = 0; t < len[m]; t++) sum[m] = fradd9(sum[m], solve_term(V, L, wtns, n_wires, s[m] + t));
    }
    unsigned long long longs = __ballot(live && total > SOLVE_SHORT);
    while (longs) {
        const int src = __ffsll((long long)longs) - 1;
        longs &= longs - 1;
#pragma unroll
        for (int m = 0; m < 3; m++) {
            const uint32_t ls = __shfl(s[m], src, 64), ll = __shfl(len[m], src, 64);
            Fr9            acc = fq9_zero();
            for (uint32_t t = lane; t < ll; t += 64u) acc = fradd9(acc, solve_term(V, L, wtns, n_wires, ls + t));
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                Fr9 o;
#pragma unroll
                for (int i = 0; i < 9; i++) o.l[i] = (uint32_t)__shfl_xor((int)acc.l[i], d, 64);
                acc = fradd9(acc, o);
            }
            if ((int)lane == src) sum[m] = acc;
        }
    }
    bool add = false;
    if (live) {
        Fr9 lin = fq9_zero();
        if (e.y != R1CS_PAIR_NONE) lin = frmul9(L.at(e.y), sum[1]);
        else if (e.z != R1CS_PAIR_NONE) lin = frmul9(L.at(e.z), sum[0]);
        if (e.w != R1CS_PAIR_NONE) lin = frsub9(lin, L.at(e.w));
        if (fr9_nonzero(lin)) {
            Fr9 one  = fq9_zero();
            one.l[0] = 1;
            const Fr9 k0  = frsub9(frmul9(sum[0], sum[1]), sum[2]);
            const Fr9 inv = frinv9(frmul9(lin, one));
            st_fr(&val[c], fr9_to_standard(frsub9(fq9_zero(), frmul9(k0, inv))));
            add = atomicMin(&by[x], c) == DET_NONE;
        }
    }
    wave_append(front, &st->n_front, n_wires, add, x);
}

// front[from .. st->n_front): the wires this round solved; by is final for them (k_r1cs_solve_derive has ended).  A workgroup
// strides them: any grid covers them.
__global__ void __launch_bounds__(256) k_r1cs_solve_commit(const uint32_t* __restrict__ front, uint32_t from, const DetState* st,
                                                           const uint32_t* __restrict__ by, const Fr* __restrict__ val, uint32_t n_wires,
                                                           uint32_t M, Fr* __restrict__ wtns)
{
    const uint32_t total = __atomic_load_n(&st->n_front, __ATOMIC_RELAXED);
    const uint32_t todo  = total > from ? total - from : 0;
    for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < todo; k += (uint64_t)gridDim.x * 256u) {
        const uint32_t x = front[from + k];
        if (x >= n_wires) continue;
        const uint32_t c = by[x];
        if (c < M) st_fr(&wtns[x], ld_fr(&val[c]));
    }
}

// verdict: the check's mask on the completed assignment.  judged / open: n_words words each; open bit c = constraint c still
// has a wire outside K, judged = verdict without those.  Lanes beyond M vote 0.  Launched with whole waves.
__global__ void __launch_bounds__(256) k_r1cs_solve_close(const unsigned long long* __restrict__ verdict, const uint32_t* __restrict__ cnt,
                                                          uint32_t M, uint32_t n_words, unsigned long long* __restrict__ judged,
                                                          unsigned long long* __restrict__ open)
{
    const uint32_t           i     = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long votes = __ballot(i < M && cnt[i] != 0u);
    if ((threadIdx.x & 63u) == 0 && (i >> 6) < n_words) {
        judged[i >> 6] = verdict[i >> 6] & ~votes;
        open[i >> 6]   = votes;
    }
}

// The bit rule of the witness completion (k16_r1cs_complete_witness_ex with K16_SOLVE_RULE_BITS).  At
// the linear rule's fixed point a constraint c with k = 2 .. 253 wires x_1 .. x_k outside K gives all of them when
//   (a) every x_j is BOOLEAN (r1cs_bools.h: the circuit itself holds it to {0, 1}),
//   (b) the unknowns with A^ != 0 and those with B^ != 0 are not both there: the residual is linear in them,
//           sum lin_j x_j + k0,   lin_j = A^_j b0 + B^_j a0 - C^_j,   k0 = a0 b0 - c0     (a0, b0, c0: the sums over K),
//   (c) with lambda = the lin of the LOWEST unknown wire or, failing that, of the HIGHEST, every lin_j / lambda is 2^(e_j) as a
//       canonical integer, the e_j distinct and at most 252.
// Then v = -k0 / lambda (canonical) must be sum 2^(e_j) x_j < 2^253 < r: a sum of distinct powers of two below r determines its
// bits, so x_j = bit e_j of v where v has no bit outside the e_j (FEASIBLE), and no 0/1 assignment exists otherwise (INFEASIBLE:
// nothing is given, the constraint's bit is set in `infeasible`).
//   k_r1cs_bits_filter   a lane per constraint: 2 <= cnt <= 253 -> the bit candidates (their own list, any order)
//   k_r1cs_solve_bits    a wave per candidate (below)
//   k_r1cs_bits_commit   a lane per frontier wire: by[x] is final, wtns[x] = the bit the row by[x] claimed
// THE COMMIT HAZARD again (two rows of a level may claim x with different bits): a wave leaves its claim in a byte of its OWN,
// claim[i] of the incidence i = (x, c) -- no two waves write one byte -- and the commit finds the incidence (x, by[x]) in x's
// column, which is ordered by constraint.  by[x] was all ones before the level, so the byte read is this level's.
// Scalings (see k_r1cs_solve_derive): coefficients k 2^522, sums s 2^261, frmul9 divides by 2^261.
//   lin_j   frmul9(A^ 2^522, b0 2^261) - C^ 2^522 = lin_j 2^522 (or B^ a0; never both, by (b); neither: -C^ alone)
//   lambda  frmul9(lambda 2^522, 1) = lambda 2^261, its R' value; frinv9 gives the R' value of the inverse, lambda^-1 2^261 =: I
//   ratio   frmul9(lin_j 2^522, I) = (lin_j / lambda) 2^522; frmul9(., 1) = (lin_j / lambda) 2^261; fr9_to_standard divides by
//           2^261 once more and reduces: the canonical integer lin_j / lambda, on which "a single bit" is a popcount
//   v       k0 2^261 = frmul9(a0 2^261, b0 2^261) - c0 2^261; frmul9(k0 2^261, I) = (k0 / lambda) 2^261, negated by
//           frsub9(0, .), fr9_to_standard: the canonical v
// Every operand is < 2r (sums by fradd9 / frsub9, products by frmul9), as in the kernels above.
constexpr uint32_t BITS_MIN = 2, BITS_MAX = 253; // unknowns of a bit row: exponents 0 .. 252
constexpr uint32_t BITS_PER_LANE = 4;            // 4 x 64 lanes >= BITS_MAX
constexpr uint32_t BITS_GRID = 2048;           // workgroups (of one wave) of k_r1cs_solve_bits / k_r1cs_det_bits

// cnt: the outside counts at the fixed point.  total: cleared before the launch.  Launched with whole waves, any grid.
__global__ void __launch_bounds__(256) k_r1cs_bits_filter(const uint32_t* __restrict__ cnt, uint32_t M, uint32_t* __restrict__ bcand, uint32_t* total)
{
    for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < M; base += (uint64_t)gridDim.x * 256u) {
        const uint64_t c = base + threadIdx.x;
        wave_append(bcand, total, M, c < M && cnt[c] >= BITS_MIN && cnt[c] <= BITS_MAX, (uint32_t)c);
    }
}

// The constraint-side index: cinc[cstart[c] .. cstart[c + 1]) are the incidences (indices into L.inc) of constraint c, by wire.
struct RowIndex {
    const uint32_t* __restrict__ cstart;
    const uint32_t* __restrict__ cinc;
};

__device__ __forceinline__ Fr9 wave_bcast9(const Fr9& a, int src)
{
    Fr9 o;
#pragma unroll
    for (int i = 0; i < 9; i++) o.l[i] = (uint32_t)__shfl((int)a.l[i], src, 64);
    return o;
}

// bcand[0 .. *n_bcand): the bit candidates of this level; ONE WAVE per workgroup, a workgroup strides the candidates.  Every
// branch below is taken by the whole wave (its condition comes from a ballot, a broadcast or a reduction), so the shuffles, the
// barriers and wave_append see all 64 lanes.
//   1  the unknown incidences are gathered through LDS in the order of the row index (by wire): slot p of the row lies in lane
//      p % 64, register p / 64 -- the lowest unknown wire in lane 0, up to BITS_PER_LANE a lane
//   2  tests (a) and (b): they need no arithmetic and end most rows that are no decomposition
//   3  the three row sums, lanes striding the row, butterfly reduction (unknown wires hold 0 in wtns: the invariant masks them)
//   4  lin_j; lambda's lane runs frinv9, the inverse is broadcast; ratio_j to canonical standard form, the single-bit test
//   5  the exponents are ORed over the wave into a 256-bit mask: its popcount is k exactly when they are distinct
//   6  v and the subset test
//   7  the claims: claim[i] = the bit, atomicMin(by[x], c), the first claim appends x to the frontier
__global__ void __launch_bounds__(64) k_r1cs_solve_bits(const uint32_t* __restrict__ bcand, const uint32_t* __restrict__ n_bcand, const IncList L,
                                                        const RowView V, const RowIndex X, const Fr* __restrict__ wtns,
                                                        const unsigned long long* __restrict__ known, const unsigned long long* __restrict__ boolean,
                                                        const uint32_t* __restrict__ cnt, uint32_t n_wires, uint32_t* by, uint8_t* __restrict__ claim,
                                                        unsigned long long* infeasible, uint32_t* __restrict__ front, DetState* st)
{
    __shared__ uint32_t slot[BITS_PER_LANE * 64];
    const uint32_t      lane = threadIdx.x & 63u;
    const uint32_t      n    = min(*n_bcand, L.M);
    for (uint32_t w = blockIdx.x; w < n; w += gridDim.x) {
        const uint32_t c = bcand[w];
        if (c >= L.M) continue;
        const uint32_t k = cnt[c];
        if (k < BITS_MIN || k > BITS_MAX) continue;
        // 1: the unknown incidences, in the order of the index
        const uint32_t cs = X.cstart[c], ce = min(X.cstart[c + 1], L.n_pairs);
        uint32_t       found = 0;
        __syncthreads(); // (the slots of the candidate before are read by now)
        for (uint32_t at = cs; at < ce; at += 64u) {
            uint32_t idx = DET_NONE;
            bool     out = false;
            if (at + lane < ce) {
                idx = X.cinc[at + lane];
                if (idx < L.n_pairs) {
                    const uint32_t x = L.wire[idx];
                    out              = x < n_wires && L.inc[idx].x == c && !det_bit(known, x);
                }
            }
            const unsigned long long votes = __ballot(out);
            const uint32_t           pos   = found + (uint32_t)__popcll(votes & ((1ull << lane) - 1));
            if (out && pos < BITS_PER_LANE * 64u) slot[pos] = idx;
            found += (uint32_t)__popcll(votes);
        }
        __syncthreads();
        if (found != k) continue; // (cnt counts exactly the incidences outside K)
        uint32_t idx[BITS_PER_LANE], x[BITS_PER_LANE];
        uint4    e[BITS_PER_LANE];
        bool     ok = true, onA = false, onB = false;
#pragma unroll
        for (uint32_t j = 0; j < BITS_PER_LANE; j++) {
            const uint32_t p = lane + 64u * j;
            idx[j]           = p < k ? slot[p] : DET_NONE;
            x[j]             = 0;
            e[j]             = make_uint4(0, R1CS_PAIR_NONE, R1CS_PAIR_NONE, R1CS_PAIR_NONE);
            if (p < k) {
                x[j] = L.wire[idx[j]];
                e[j] = L.inc[idx[j]];
                ok   = ok && det_bit(boolean, x[j]);          // (a)
                onA  = onA || e[j].y != R1CS_PAIR_NONE;
                onB  = onB || e[j].z != R1CS_PAIR_NONE;
            }
        }
        // 2: (a), and (b): unknowns on A and unknowns on B (one wire on both included) leave a product of unknowns
        if (__ballot(!ok) || (__ballot(onA) && __ballot(onB))) continue;
        // 3: the row sums, in every lane
        Fr9 sum[3];
#pragma unroll
        for (int m = 0; m < 3; m++) {
            const uint32_t ls = V.start[(size_t)m * L.M + c], le = V.start[(size_t)m * L.M + c + 1];
            Fr9            acc = fq9_zero();
            for (uint64_t t = (uint64_t)ls + lane; t < le; t += 64u) acc = fradd9(acc, solve_term(V, L, wtns, n_wires, (uint32_t)t));
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                Fr9 o;
#pragma unroll
                for (int i = 0; i < 9; i++) o.l[i] = (uint32_t)__shfl_xor((int)acc.l[i], d, 64);
                acc = fradd9(acc, o);
            }
            sum[m] = wave_bcast9(acc, 0); // one representative of the sum for the whole wave
        }
        // 4: lin_j 2^522
        Fr9 one  = fq9_zero();
        one.l[0] = 1;
        Fr9 lin[BITS_PER_LANE];
#pragma unroll
        for (uint32_t j = 0; j < BITS_PER_LANE; j++) {
            lin[j] = fq9_zero();
            if (e[j].y != R1CS_PAIR_NONE) lin[j] = frmul9(L.at(e[j].y), sum[1]);
            else if (e[j].z != R1CS_PAIR_NONE) lin[j] = frmul9(L.at(e[j].z), sum[0]);
            if (e[j].w != R1CS_PAIR_NONE) lin[j] = frsub9(lin[j], L.at(e[j].w));
        }
        const Fr9 k0 = frsub9(frmul9(sum[0], sum[1]), sum[2]);
        // lambda: the lin of slot 0 (the lowest unknown wire), then of slot k - 1 (the highest)
        bool     solved = false;
        Fr9      inv    = fq9_zero();
        uint32_t ex[BITS_PER_LANE] = {0, 0, 0, 0};
        uint32_t mask[8];
        for (uint32_t attempt = 0; attempt < 2 && !solved; attempt++) {
            const uint32_t p = attempt == 0 ? 0u : k - 1u, src = p & 63u, reg = p >> 6;
            Fr9            lam = lin[0];
#pragma unroll
            for (uint32_t j = 1; j < BITS_PER_LANE; j++)
                if (reg == j) lam = lin[j];
            lam = wave_bcast9(lam, (int)src);
            if (!fr9_nonzero(lam)) continue; // (the same value in every lane)
            if (lane == src) inv = frinv9(frmul9(lam, one));
            inv = wave_bcast9(inv, (int)src);
            bool fits = true;
#pragma unroll
            for (int i = 0; i < 8; i++) mask[i] = 0;
#pragma unroll
            for (uint32_t j = 0; j < BITS_PER_LANE; j++) {
                if (lane + 64u * j >= k) continue;
                const Fr ratio = fr9_to_standard(frmul9(frmul9(lin[j], inv), one));
                uint32_t pop = 0, at = 0;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    pop += (uint32_t)__popc(ratio.v[i]);
                    if (ratio.v[i]) at = 32u * i + (uint32_t)__ffs((int)ratio.v[i]) - 1u;
                }
                if (pop != 1u || at >= BITS_MAX) {
                    fits = false;
                    continue;
                }
                ex[j] = at;
#pragma unroll
                for (int i = 0; i < 8; i++)
                    if ((at >> 5) == (uint32_t)i) mask[i] |= 1u << (at & 31u);
            }
            if (__ballot(!fits)) continue;
            // 5: distinct exponents
            uint32_t pop = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) {
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) mask[i] |= (uint32_t)__shfl_xor((int)mask[i], d, 64);
                pop += (uint32_t)__popc(mask[i]);
            }
            solved = pop == k;
        }
        if (!solved) continue;
        // 6: v = -k0 / lambda, canonical; FEASIBLE when it has no bit outside the exponents (then v < 2^253 as well)
        const Fr v       = fr9_to_standard(frsub9(fq9_zero(), frmul9(k0, inv)));
        uint32_t outside = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) outside |= v.v[i] & ~mask[i];
        if (outside) {
            if (lane == 0) atomicOr(&infeasible[c >> 6], 1ull << (c & 63u));
            continue;
        }
        // 7: the claims
#pragma unroll
        for (uint32_t j = 0; j < BITS_PER_LANE; j++) {
            bool add = false;
            if (lane + 64u * j < k) {
                uint32_t word = 0;
#pragma unroll
                for (int i = 0; i < 8; i++)
                    if ((ex[j] >> 5) == (uint32_t)i) word = v.v[i];
                claim[idx[j]] = (uint8_t)((word >> (ex[j] & 31u)) & 1u);
                add           = atomicMin(&by[x[j]], c) == DET_NONE;
            }
            wave_append(front, &st->n_front, n_wires, add, x[j]);
        }
    }
}

// front[from .. st->n_front): the wires this bit level solved; by is final for them (k_r1cs_solve_bits has ended).  The incidence
// (x, by[x]) is found by bisection in x's column (start: the closure's column starts) and its claim goes into wtns.  A workgroup
// strides the wires: any grid covers them.
__global__ void __launch_bounds__(256) k_r1cs_bits_commit(const uint32_t* __restrict__ front, uint32_t from, const DetState* st,
                                                          const uint32_t* __restrict__ by, const uint32_t* __restrict__ start, const IncList L,
                                                          const uint8_t* __restrict__ claim, uint32_t n_wires, uint4* __restrict__ wtns)
{
    const uint32_t total = __atomic_load_n(&st->n_front, __ATOMIC_RELAXED);
    const uint32_t todo  = total > from ? total - from : 0;
    for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < todo; k += (uint64_t)gridDim.x * 256u) {
        const uint32_t x = front[from + k];
        if (x >= n_wires) continue;
        const uint32_t c  = by[x];
        uint32_t       lo = start[x], hi = min(start[x + 1], L.n_pairs);
        while (lo < hi) { // the first incidence of the column whose constraint is not below c
            const uint32_t mid = lo + (hi - lo) / 2;
            if (L.inc[mid].x < c) lo = mid + 1;
            else hi = mid;
        }
        if (lo < min(start[x + 1], L.n_pairs) && L.inc[lo].x == c) {
            wtns[2 * (size_t)x]     = make_uint4(claim[lo], 0, 0, 0);
            wtns[2 * (size_t)x + 1] = make_uint4(0, 0, 0, 0);
        }
    }
}

// The bit rule of the determinism closure (k16_r1cs_determined_wires_ex with K16_DET_RULE_BITS).  The
// closure reads the sums and the verdicts of the last completed check, never the witness, so "x is 0 or 1 in this witness" has to
// come from there as well: a wire x >= 1 is HELD when some marking row of x (r1cs_bools.h) is not broken -- its residual
// quad x (x - 1) is 0 with quad != 0.  HELD is a subset of BOOLEAN and all of it on a satisfying witness.
// At the PIN rule's fixed point an unbroken constraint c with k = 2 .. 253 wires x_1 .. x_k outside K gives all of them when
//   (a) every x_j is HELD,
//   (b) no outside incidence names A^ or none names B^ (one wire on both sides counts as both): the sum of d_rows that
//       multiplies an unknown is then a sum over K, and inc_terms' lin_j = A^_j b0 + B^_j a0 - C^_j depends on K alone,
//   (c) as the completion's (c): lambda = the lin of the LOWEST outside wire, else of the HIGHEST, 0 is no lambda; every
//       lin_j / lambda is 2^(e_j) as a canonical integer, the e_j distinct and at most 252.
// SOUND: let w' satisfy the circuit and agree with this witness w on K.  w'_j is 0 or 1 by the static marks, w_j by HELD; both
// residuals of c are 0 and differ by lambda sum 2^(e_j) (w_j - w'_j): that sum is 0 modulo r, below 2^253 < r in absolute value,
// so 0 as an integer, and two 0/1 vectors with the same sum over distinct powers of two are equal.  There is no feasibility test:
// c is unbroken and the x_j are 0/1, so the witness IS the expansion.  Three things that are no inefficiency:
//   a BROKEN c derives nothing                        its residual is not 0: the difference of the residuals says nothing
//   a BOOLEAN wire whose marking rows are all broken  is not HELD: its value here need not be 0 or 1
//   a FREE outside incidence (lin_j = 0)              fails (c), whichever end lambda comes from, and keeps the row out
//   k_r1cs_held         a lane per marking row: not broken -> its wire's bit in `held` (cleared before the launch; an OR)
//   k_r1cs_bits_filter  the completion's, unchanged
//   k_r1cs_det_bits     a wave per candidate, the shape of k_r1cs_solve_bits without the row sums, v, the claims and the commit
//   k_r1cs_det_expand   the closure's, on the frontier the level appended
// by[x] is a minimum over the rows that qualify with respect to the level before (`known` and cnt are only read here), the rule
// byte is written by the one lane that found by[x] empty, and no two levels write one wire: nothing depends on the launch order.
__global__ void __launch_bounds__(256) k_r1cs_held(const uint32_t* __restrict__ row, const uint32_t* __restrict__ row_wire, uint32_t n,
                                                   const unsigned long long* __restrict__ verdict, uint32_t M, uint32_t n_wires,
                                                   unsigned long long* held)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = row[i], x = row_wire[i];
    if (c >= M || x >= n_wires || det_bit(verdict, c)) return;
    const unsigned long long bit = 1ull << (x & 63u);
    if (!(__atomic_load_n(&held[x >> 6], __ATOMIC_RELAXED) & bit)) atomicOr(&held[x >> 6], bit); // (bits are only ever set)
}

// bcand[0 .. *n_bcand): the bit candidates of this level; ONE WAVE per workgroup, a workgroup strides the candidates, every
// branch is taken by the whole wave, as in k_r1cs_solve_bits.  rule: n_wires bytes, cleared before the first level.
//   1  the verdict of c, then the gather of the unknown incidences through LDS: slot p in lane p % 64, register p / 64
//   2  tests (a) and (b): no arithmetic so far
//   3  lin_j 2^522 from inc_terms: the check's sums, no row is walked
//   4  lambda's lane runs frinv9, the inverse is broadcast; ratio_j to canonical standard form, the single-bit test
//   5  the exponents ORed over the wave into a 256-bit mask: its popcount is k exactly when they are distinct
//   6  atomicMin(by[x], c); the lane that found it empty appends x to the frontier and writes the rule byte
__global__ void __launch_bounds__(64) k_r1cs_det_bits(const uint32_t* __restrict__ bcand, const uint32_t* __restrict__ n_bcand, const IncList L,
                                                      const RowIndex X, const unsigned long long* __restrict__ verdict,
                                                      const unsigned long long* __restrict__ known, const unsigned long long* __restrict__ held,
                                                      const uint32_t* __restrict__ cnt, uint32_t n_wires, uint32_t* by, uint8_t* __restrict__ rule,
                                                      uint32_t* __restrict__ front, DetState* st)
{
    __shared__ uint32_t slot[BITS_PER_LANE * 64];
    const uint32_t      lane = threadIdx.x & 63u;
    const uint32_t      n    = min(*n_bcand, L.M);
    for (uint32_t w = blockIdx.x; w < n; w += gridDim.x) {
        const uint32_t c = bcand[w];
        if (c >= L.M || det_bit(verdict, c)) continue; // a broken row derives nothing
        const uint32_t k = cnt[c];
        if (k < BITS_MIN || k > BITS_MAX) continue;
        // 1: the unknown incidences, in the order of the index
        const uint32_t cs = X.cstart[c], ce = min(X.cstart[c + 1], L.n_pairs);
        uint32_t       found = 0;
        __syncthreads(); // (the slots of the candidate before are read by now)
        for (uint32_t at = cs; at < ce; at += 64u) {
            uint32_t idx = DET_NONE;
            bool     out = false;
            if (at + lane < ce) {
                idx = X.cinc[at + lane];
                if (idx < L.n_pairs) {
                    const uint32_t x = L.wire[idx];
                    out              = x < n_wires && L.inc[idx].x == c && !det_bit(known, x);
                }
            }
            const unsigned long long votes = __ballot(out);
            const uint32_t           pos   = found + (uint32_t)__popcll(votes & ((1ull << lane) - 1));
            if (out && pos < BITS_PER_LANE * 64u) slot[pos] = idx;
            found += (uint32_t)__popcll(votes);
        }
        __syncthreads();
        if (found != k) continue; // (cnt counts exactly the incidences outside K)
        uint32_t x[BITS_PER_LANE];
        uint4    e[BITS_PER_LANE];
        bool     ok = true, onA = false, onB = false;
#pragma unroll
        for (uint32_t j = 0; j < BITS_PER_LANE; j++) {
            const uint32_t p = lane + 64u * j;
            x[j]             = 0;
            e[j]             = make_uint4(0, R1CS_PAIR_NONE, R1CS_PAIR_NONE, R1CS_PAIR_NONE);
            if (p < k) {
                const uint32_t idx = slot[p];
                x[j]               = L.wire[idx];
                e[j]               = L.inc[idx];
                ok                 = ok && det_bit(held, x[j]);   // (a)
                onA                = onA || e[j].y != R1CS_PAIR_NONE;
                onB                = onB || e[j].z != R1CS_PAIR_NONE;
            }
        }
        // 2: (a), and (b): with unknowns on A and unknowns on B (one wire on both included) the sums are not sums over K
        if (__ballot(!ok) || (__ballot(onA) && __ballot(onB))) continue;
        // 3: lin_j 2^522; by (b) no incidence here names both sides
        Fr9 one  = fq9_zero();
        one.l[0] = 1;
        Fr9 lin[BITS_PER_LANE];
#pragma unroll
        for (uint32_t j = 0; j < BITS_PER_LANE; j++) lin[j] = lane + 64u * j < k ? inc_terms(e[j], L).lin : fq9_zero();
        // 4: lambda: the lin of slot 0 (the lowest unknown wire), then of slot k - 1 (the highest)
        bool solved = false;
        for (uint32_t attempt = 0; attempt < 2 && !solved; attempt++) {
            const uint32_t p = attempt == 0 ? 0u : k - 1u, src = p & 63u, reg = p >> 6;
            Fr9            lam = lin[0];
#pragma unroll
            for (uint32_t j = 1; j < BITS_PER_LANE; j++)
                if (reg == j) lam = lin[j];
            lam = wave_bcast9(lam, (int)src);
            if (!fr9_nonzero(lam)) continue; // (the same value in every lane)
            Fr9 inv = fq9_zero();
            if (lane == src) inv = frinv9(frmul9(lam, one));
            inv = wave_bcast9(inv, (int)src);
            bool     fits = true;
            uint32_t mask[8];
#pragma unroll
            for (int i = 0; i < 8; i++) mask[i] = 0;
#pragma unroll
            for (uint32_t j = 0; j < BITS_PER_LANE; j++) {
                if (lane + 64u * j >= k) continue;
                const Fr ratio = fr9_to_standard(frmul9(frmul9(lin[j], inv), one));
                uint32_t pop = 0, at = 0;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    pop += (uint32_t)__popc(ratio.v[i]);
                    if (ratio.v[i]) at = 32u * i + (uint32_t)__ffs((int)ratio.v[i]) - 1u;
                }
                if (pop != 1u || at >= BITS_MAX) {
                    fits = false;
                    continue;
                }
#pragma unroll
                for (int i = 0; i < 8; i++)
                    if ((at >> 5) == (uint32_t)i) mask[i] |= 1u << (at & 31u);
            }
            if (__ballot(!fits)) continue;
            // 5: distinct exponents
            uint32_t pop = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) {
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) mask[i] |= (uint32_t)__shfl_xor((int)mask[i], d, 64);
                pop += (uint32_t)__popc(mask[i]);
            }
            solved = pop == k;
        }
        if (!solved) continue;
        // 6: every x_j joins K
#pragma unroll
        for (uint32_t j = 0; j < BITS_PER_LANE; j++) {
            bool add = false;
            if (lane + 64u * j < k) {
                add = atomicMin(&by[x[j]], c) == DET_NONE;
                if (add) rule[x[j]] = (uint8_t)K16_DET_RULE_BITS;
            }
            wave_append(front, &st->n_front, n_wires, add, x[j]);
        }
    }
}

// The open-set solve (k16_r1cs_open_system, k16_r1cs_open_direction): rank and null space of what a
// closure leaves open.  The host (r1cs_open.h) cuts the outside wires into components and lists, per component of at most 64
// wires, its LINEAR rows; the matrix J of a component has those rows, the component's wires (ascending) as columns and the
// incidences' lin as entries.  k_r1cs_open_rref brings J to its reduced row echelon form R, ONE WAVE per component, lane j
// owning column j.  A wire x is FORCED when e_x lies in the row space: x is a pivot column and its row of R is zero in every
// non-pivot column.
//   the basis      rank rows, kept REDUCED at every step (a 1 in the own pivot column, 0 in every other pivot column), in LDS
//                  as basis[row][limb][column]: the lanes of a wave read and write neighbouring banks
//   a row of J     its entries are computed lane-parallel (inc_terms) and scattered into a zeroed row vector in LDS; lane j
//                  then holds entry j.  Reduced against the basis: the factors are the row's OWN entries in the pivot columns
//                  (the basis being reduced, no factor depends on another subtraction): rank multiply-subtracts per lane
//   the remainder  zero mod r in every column (fr9_nonzero: lazy representatives below 2r) -> the row is discarded; else its
//                  lowest non-zero column p becomes a pivot (ballot, count): lane p runs frinv9, the inverse is broadcast, the
//                  row is normalised, column p is cleared from every basis row, the row is inserted.  Pivots are leading
//                  entries: a basis row is zero below its pivot when it enters, and every later row added to it starts at a
//                  higher column or has factor zero -- so the end state is THE reduced row echelon form, whatever the row order
// Every loop bound is a count the host wrote (components, rows, entries) or the rank, which grows by one per inserted row and
// cannot pass the number of columns.  Nothing iterates until nothing changes.
// Scalings: inc_terms gives lin 2^522 = (lin 2^261) 2^261, the R' value of lin 2^261.  Every row of J carries the same extra
// factor 2^261, which changes neither row space nor R; the elimination is plain R' arithmetic (frmul9 of two R' values is the
// R' value of the product, frinv9 of an R' value that of the inverse).  Operands: sums and differences < 2r by fradd9 / frsub9,
// products < 2r by frmul9.  An entry of R leaves through fr9_to_standard: canonical standard form.
// With `emit` (one component, k16_r1cs_open_direction) the canonical direction d of column emit_col is written as 64 values:
//   F the free columns; v_f[f] = 1, v_f[f'] = 0, v_f[p] = -R[row(p)][f];  x free: d = v_x;  x a pivot: f = the lowest free column
//   with R[row(x)][f] != 0 and d = v_f / v_f[x] (one more inversion, on lane x).  All zero where x is FORCED.
struct OpenJob {
    const R1csOpenComp* __restrict__ comp;       // the components of this launch
    uint32_t n_comp;
    const uint32_t* __restrict__ row_start;      // [n_rows + 1]
    const uint2* __restrict__ ent;               // [n_ent] (column, incidence)
    uint32_t n_rows, n_ent, n_wires;             // the sizes of row_start, ent and cls: nothing is read or written beyond them
    unsigned long long* __restrict__ out;        // per component of the launch: rank | pivot mask | FORCED mask
    uint8_t* __restrict__ cls;                   // [n_wires] by position in the work list's wires
    Fr* __restrict__ emit;                       // null, or 64 values
    uint32_t emit_col;
};
static_assert(sizeof(R1csOpenComp) == 24 && sizeof(R1csOpenEntry) == sizeof(uint2), "the work list is uploaded as it is");

template <uint32_t W>
__global__ void __launch_bounds__(64) k_r1cs_open_rref(const IncList L, const OpenJob J)
{
    __shared__ uint32_t basis[W * 9 * W]; // [(row * 9 + limb) * W + column]
    __shared__ uint32_t rowv[9 * W];      // [limb * W + column]
    const uint32_t lane = threadIdx.x & 63u;
    const bool     mine = lane < W; // (lanes beyond the class's width hold no column)
    const uint32_t own_col = mine ? lane : 0u; // what such a lane may index the basis with: no load leaves the array, used or not
    auto load_basis = [&](uint32_t row, uint32_t col) {
        Fr9 b;
#pragma unroll
        for (int i = 0; i < 9; i++) b.l[i] = basis[(row * 9u + i) * W + col];
        return b;
    };
    for (uint32_t k = blockIdx.x; k < J.n_comp; k += gridDim.x) {
        const R1csOpenComp C  = J.comp[k];
        const uint32_t     nw = min(C.n_wires, W);
        const bool         col = lane < nw;
        uint32_t           rank = 0, my_pivot = 0, my_row = 0; // lane k: the pivot of basis row k; lane j: the row of pivot column j
        unsigned long long pivots = 0;
        for (uint32_t r = 0; r < C.n_rows; r++) {
            if (C.row0 + r >= J.n_rows) break; // (the same in every lane)
            const uint32_t rs = J.row_start[C.row0 + r], re = min(J.row_start[C.row0 + r + 1], J.n_ent);
            const uint32_t len = re > rs ? min(re - rs, W) : 0;
            __syncthreads(); // (the row before is read by now)
            if (mine) {
#pragma unroll
                for (int i = 0; i < 9; i++) rowv[i * W + lane] = 0;
            }
            __syncthreads();
            if (lane < len) {
                const uint2 e = J.ent[rs + lane];
                if (e.x < nw && e.y < L.n_pairs) {
                    const IncTerms t = inc_terms(L.inc[e.y], L);
#pragma unroll
                    for (int i = 0; i < 9; i++) rowv[i * W + e.x] = t.lin.l[i];
                }
            }
            __syncthreads();
            Fr9 v = fq9_zero();
            if (mine) {
#pragma unroll
                for (int i = 0; i < 9; i++) v.l[i] = rowv[i * W + lane];
            }
            const Fr9 own = v;
            for (uint32_t b = 0; b < rank; b++) {
                const Fr9 f = wave_bcast9(own, (int)__shfl(my_pivot, (int)b, 64));
                if (mine) v = frsub9(v, frmul9(f, load_basis(b, lane)));
            }
            const unsigned long long live = __ballot(col && !((pivots >> lane) & 1ull) && fr9_nonzero(v));
            if (!live || rank >= W) continue; // in the row space already
            const uint32_t p = (uint32_t)__ffsll((long long)live) - 1u;
            Fr9            inv = fq9_zero();
            if (lane == p) inv = frinv9(v);
            inv = wave_bcast9(inv, (int)p);
            v   = frmul9(v, inv);
            for (uint32_t b = 0; b < rank; b++) {
                const Fr9 f = load_basis(b, p); // (one address for the wave: a broadcast read)
                if (mine) {
                    const Fr9 c = frsub9(load_basis(b, lane), frmul9(f, v));
#pragma unroll
                    for (int i = 0; i < 9; i++) basis[(b * 9u + i) * W + lane] = c.l[i];
                }
            }
            if (mine) {
#pragma unroll
                for (int i = 0; i < 9; i++) basis[(rank * 9u + i) * W + lane] = v.l[i];
            }
            if (lane == rank) my_pivot = p;
            if (lane == p) my_row = rank;
            pivots |= 1ull << p;
            rank++;
        }
        __syncthreads();
        // FORCED: a pivot whose row is zero in every free column
        unsigned long long forced = 0;
        for (uint32_t b = 0; b < rank; b++) {
            const uint32_t p = __shfl(my_pivot, (int)b, 64);
            if (!__ballot(col && !((pivots >> lane) & 1ull) && fr9_nonzero(load_basis(b, own_col)))) forced |= 1ull << p;
        }
        if (lane == 0) {
            J.out[3 * (size_t)k]     = rank;
            J.out[3 * (size_t)k + 1] = pivots;
            J.out[3 * (size_t)k + 2] = forced;
        }
        if (col && (uint64_t)C.wire0 + lane < J.n_wires)
            J.cls[C.wire0 + lane] = (uint8_t)((forced >> lane) & 1ull ? K16_OPEN_FORCED : C.n_cross ? K16_OPEN_UNDECIDED : K16_OPEN_FREE);
        if (J.emit) {
            const uint32_t x    = min(J.emit_col, 63u);
            uint32_t       f    = x;
            bool           have = x < nw && !((forced >> x) & 1ull);
            const bool     on_pivot = (pivots >> x) & 1ull;
            if (on_pivot) { // the lowest free column in x's row
                const uint32_t           row  = __shfl(my_row, (int)x, 64);
                const unsigned long long free = __ballot(col && !((pivots >> lane) & 1ull) && row < rank && fr9_nonzero(load_basis(row < rank ? row : 0u, own_col)));
                have = have && free != 0;
                f    = free ? (uint32_t)__ffsll((long long)free) - 1u : 0u;
            }
            Fr9 d = fq9_zero();
            if (have && col) {
                if (lane == f) d = fr9_one();
                else if ((pivots >> lane) & 1ull) d = frsub9(fq9_zero(), load_basis(my_row, f));
            }
            if (have && on_pivot) { // (the same branch in every lane)
                Fr9 inv = fq9_zero();
                if (lane == x) inv = frinv9(d);
                d = frmul9(d, wave_bcast9(inv, (int)x));
            }
            st_fr(&J.emit[lane], fr9_to_standard(d));
        }
    }
}

// The wide classes of the open-set solve (k16_r1cs_open_system_ex / k16_r1cs_open_direction_ex with max_wires > 64; DESIGN.md
// section 10i): components of 65 .. 128 and 129 .. 256 wires.  Definitions, work list, scalings and operand bounds are those of
// k_r1cs_open_rref above.  ONE WORKGROUP of W threads (W / 64 waves) per component, thread j owning column j; a workgroup
// strides the components of its class.
//   the basis      in a global slab per WORKGROUP, slab[(row * 9 + limb) * W + column], W * 9 * W words.  A thread reads and
//                  writes ITS OWN COLUMN of the slab and nothing else, so no store of one wave is ever read by another through
//                  global memory; what crosses threads goes through LDS between workgroup barriers.  A slab row is written in
//                  all W columns when it is inserted, before anything reads it: nothing is zeroed between components
//   fraction-free  the basis rows are REDUCED BUT NOT NORMALISED: row b holds some p_b != 0 in its own pivot column c_b and 0
//                  in every other pivot column, so basis_b = p_b R_b for the row R_b of the reduced row echelon form.  A row v
//                  of J is reduced by cross-multiplication, v <- p_b v - v[c_b] basis_b, for the pivot columns among the row's
//                  OWN ENTRIES only (a column the row has no entry in holds an exact zero and stays zero: basis_b is 0 in the
//                  other pivot columns).  v[c_b] at the time of the step is the row's ORIGINAL entry (from LDS) times the
//                  product P of the p_b of the steps before it, which every thread carries redundantly: no step waits for
//                  another and the loop over the entries holds no barrier.  A remainder that is zero mod r in every non-pivot
//                  column (fr9_nonzero on lazy representatives) is discarded.  Else the lowest non-zero column p (ballot per
//                  wave, minimum over the waves through LDS) becomes a pivot with s = v[p]: basis_b <- s basis_b - basis_b[p] v
//                  for the rows with basis_b[p] != 0 (a factor whose words are all zero skips its row: nothing to clear, and
//                  no scaling is owed), which lifts p_b to s p_b; the remainder is inserted as it is, p_rank = s.  Scaling a
//                  row by a non-zero value changes no zero pattern: pivots are leading entries as above, and pivots, rank,
//                  the FORCED mask and the class bytes are those of the reduced row echelon form.  NO INVERSION.
//   through LDS    the row (rowv) and the columns of its entries (ecol), the basis row of a pivot column (rowof), the pivot
//                  values (pval: written by the thread of the pivot column, which holds p_b in its own column), the new pivot's
//                  column of the basis rows (fcol: thread p gathers it from its own column), the waves' lowest live columns
//                  (wmin), the rows with a non-zero free column (busy), what thread emit_col knows of its column (info), and
//                  per basis row a mask of the columns that hold a non-zero word (nzm: a ballot per wave whenever the row is
//                  stored; it may name a column whose value is zero mod r, never miss one that is not), from which the rows a
//                  new pivot's column has to be cleared from are listed (hitm): thread p gathers those rows only
//   no hangs       every loop bound is a count the host wrote (components, rows, entries) or the rank, which grows by one per
//                  inserted row and cannot pass W; every __syncthreads() sits in control flow that is uniform over the
//                  workgroup -- "this row is in the row space, skip it" is decided from wmin, which every thread reads after a
//                  barrier, never per wave; every index read from the work list is clamped as in k_r1cs_open_rref, so a wrong
//                  list reads and writes nothing outside a buffer
// out: 9 words per component, rank | pivot mask [4] | FORCED mask [4].  With `emit` (one component) the canonical direction of
// column emit_col is written as W values: every pivot thread inverts ITS OWN pivot value, all at once (one inversion's latency,
// whatever the rank), v_f[p] = -basis[row(p)][f] / p_row(p) with basis[.][f] gathered by thread f through LDS; where emit_col
// is a pivot its thread runs one more inversion, broadcast through LDS.
template <uint32_t W>
__global__ void __launch_bounds__(W) k_r1cs_open_rref_wide(const IncList L, const OpenJob J, uint32_t* __restrict__ slabs)
{
    constexpr uint32_t WAVES = W / 64u, NONE = 0xffffffffu;
    __shared__ uint32_t rowv[9 * W]; // [limb * W + column]
    __shared__ uint32_t fcol[9 * W]; // [row * 9 + limb]: basis[row][p] of the pivot p being inserted (emit: of column f)
    __shared__ uint32_t pval[9 * W]; // [row * 9 + limb]: p_b
    __shared__ uint32_t sval[9];
    __shared__ uint32_t ecol[W];     // the columns of the row's entries, NONE where the list names none
    __shared__ uint32_t rowof[W];    // the basis row of a pivot column, NONE for a free one
    __shared__ uint32_t busy[W];     // != 0: basis row b has a non-zero free column
    __shared__ uint32_t wmin[WAVES];
    __shared__ uint32_t info[3];
    __shared__ unsigned long long nzm[W * WAVES]; // [row * WAVES + wave]: bit l -- column 64 wave + l of the row holds a non-zero word
    __shared__ unsigned long long hitm[WAVES];    // bit b: basis row b has such a word in the column of the new pivot
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t* const slab = slabs + (size_t)blockIdx.x * (W * 9u * W) + tid; // this thread's column
    auto load_own = [&](uint32_t row) {
        Fr9 b;
#pragma unroll
        for (int i = 0; i < 9; i++) b.l[i] = slab[(row * 9u + i) * W];
        return b;
    };
    auto store_own = [&](uint32_t row, const Fr9& b) {
#pragma unroll
        for (int i = 0; i < 9; i++) slab[(row * 9u + i) * W] = b.l[i];
    };
    auto store_marked = [&](uint32_t row, const Fr9& b) { // by every thread of the workgroup: the row's mask follows its words
        store_own(row, b);
        const unsigned long long m = __ballot((b.l[0] | b.l[1] | b.l[2] | b.l[3] | b.l[4] | b.l[5] | b.l[6] | b.l[7] | b.l[8]) != 0);
        if (lane == 0) nzm[row * WAVES + wave] = m;
    };
    auto marked = [&](uint32_t row, uint32_t column) { return (nzm[row * WAVES + (column >> 6)] >> (column & 63u)) & 1ull; };
    auto load_lds = [&](const uint32_t* at, uint32_t stride) {
        Fr9 b;
#pragma unroll
        for (int i = 0; i < 9; i++) b.l[i] = at[i * stride];
        return b;
    };
    // the lowest thread with `live`, NONE when there is none: the same value in every thread.  Two barriers, uniform.
    auto lowest = [&](bool live) {
        const unsigned long long m = __ballot(live);
        __syncthreads(); // (wmin is read by now)
        if (lane == 0) wmin[wave] = m ? 64u * wave + (uint32_t)__ffsll((long long)m) - 1u : NONE;
        __syncthreads();
        uint32_t p = NONE;
#pragma unroll
        for (uint32_t i = 0; i < WAVES; i++) p = min(p, wmin[i]);
        return p;
    };
    for (uint32_t k = blockIdx.x; k < J.n_comp; k += gridDim.x) {
        const R1csOpenComp C  = J.comp[k];
        const uint32_t     nw = min(C.n_wires, W);
        const bool         col = tid < nw;
        uint32_t           rank = 0, my_row = 0; // my_row: the basis row of this thread's column, where it is a pivot
        bool               pivot = false;
        rowof[tid] = NONE; // (the component before is done with it: the barriers of its FORCED pass lie between)
        for (uint32_t r = 0; r < C.n_rows; r++) {
            if (C.row0 + r >= J.n_rows) break; // (the same in every thread)
            const uint32_t rs = J.row_start[C.row0 + r], re = min(J.row_start[C.row0 + r + 1], J.n_ent);
            const uint32_t len = re > rs ? min(re - rs, W) : 0;
            __syncthreads(); // (the row before is read by now)
#pragma unroll
            for (int i = 0; i < 9; i++) rowv[i * W + tid] = 0;
            ecol[tid] = NONE;
            __syncthreads();
            if (tid < len) {
                const uint2 e = J.ent[rs + tid];
                if (e.x < nw && e.y < L.n_pairs) {
                    const IncTerms t = inc_terms(L.inc[e.y], L);
#pragma unroll
                    for (int i = 0; i < 9; i++) rowv[i * W + e.x] = t.lin.l[i];
                    ecol[tid] = e.x;
                }
            }
            __syncthreads();
            Fr9  v = load_lds(&rowv[tid], W), P = fr9_one();
            bool first = true; // (P is 1: the first step multiplies nothing by it)
            for (uint32_t e = 0; e < len; e++) { // every condition below is the same in every thread: read from LDS
                const uint32_t c = ecol[e];
                if (c >= W) continue;
                const uint32_t b = rowof[c];
                if (b >= rank) continue; // a free column
                const Fr9 o = load_lds(&rowv[c], W), pb = load_lds(&pval[b * 9u], 1);
                const Fr9 f = first ? o : frmul9(o, P);
                v     = frsub9(frmul9(pb, v), frmul9(f, load_own(b)));
                P     = first ? pb : frmul9(P, pb);
                first = false;
            }
            const uint32_t p = lowest(col && !pivot && fr9_nonzero(v));
            if (p == NONE || rank >= W) continue; // in the row space already: every thread read the same wmin
            const unsigned long long hit = __ballot(tid < rank && marked(tid, p)); // the rows column p may have to be cleared from
            if (lane == 0) hitm[wave] = hit;
            __syncthreads();
            if (tid == p) {
#pragma unroll
                for (int i = 0; i < 9; i++) sval[i] = pval[rank * 9u + i] = v.l[i];
                for (uint32_t wv = 0; wv < WAVES; wv++)
                    for (unsigned long long m = hitm[wv]; m; m &= m - 1) {
                        const uint32_t b = 64u * wv + (uint32_t)__ffsll((long long)m) - 1u;
                        const Fr9      f = load_own(b);
#pragma unroll
                        for (int i = 0; i < 9; i++) fcol[b * 9u + i] = f.l[i];
                    }
                rowof[p] = rank;
                pivot    = true;
                my_row   = rank;
            }
            __syncthreads();
            const Fr9 s = load_lds(sval, 1);
            for (uint32_t wv = 0; wv < WAVES; wv++)
                for (unsigned long long m = hitm[wv]; m; m &= m - 1) { // (every thread alike: hitm and fcol are read from LDS)
                    const uint32_t b = 64u * wv + (uint32_t)__ffsll((long long)m) - 1u;
                    const Fr9      f = load_lds(&fcol[b * 9u], 1);
                    if (!(f.l[0] | f.l[1] | f.l[2] | f.l[3] | f.l[4] | f.l[5] | f.l[6] | f.l[7] | f.l[8])) continue;
                    const Fr9 c = frsub9(frmul9(s, load_own(b)), frmul9(f, v));
                    store_marked(b, c);
                    if (pivot && my_row == b && tid != p) { // this thread's column holds p_b: s p_b now
#pragma unroll
                        for (int i = 0; i < 9; i++) pval[b * 9u + i] = c.l[i];
                    }
                }
            store_marked(rank, v);
            rank++;
        }
        // FORCED: a pivot whose row is zero in every free column
        __syncthreads();
        busy[tid] = 0;
        __syncthreads();
        if (col && !pivot)
            for (uint32_t b = 0; b < rank; b++)
                if (marked(b, tid) && fr9_nonzero(load_own(b))) busy[b] = 1; // (every writer writes the same word)
        __syncthreads();
        const bool               forced = pivot && !busy[my_row];
        const unsigned long long pm = __ballot(pivot), fm = __ballot(forced);
        unsigned long long*      out = J.out + 9 * (size_t)k;
        if (lane == 0) {
            out[1 + wave] = pm;
            out[5 + wave] = fm;
        }
        if (tid == 0) {
            out[0] = rank;
            for (uint32_t i = WAVES; i < 4; i++) out[1 + i] = out[5 + i] = 0;
        }
        if (col && (uint64_t)C.wire0 + tid < J.n_wires)
            J.cls[C.wire0 + tid] = (uint8_t)(forced ? K16_OPEN_FORCED : C.n_cross ? K16_OPEN_UNDECIDED : K16_OPEN_FREE);
        if (J.emit) {
            const uint32_t x = min(J.emit_col, W - 1u);
            if (tid == x) {
                info[0] = pivot;
                info[1] = forced;
                info[2] = my_row;
            }
            __syncthreads();
            const bool     on_pivot = info[0] != 0;
            const uint32_t row      = min(info[2], W - 1u);
            bool           have     = x < nw && !info[1];
            uint32_t       f        = x;
            if (on_pivot) { // (the same branch in every thread) the lowest free column in x's row
                f    = lowest(col && !pivot && row < rank && fr9_nonzero(load_own(row < rank ? row : 0u)));
                have = have && f != NONE;
            }
            Fr9 d = fq9_zero();
            if (have) { // (the same branch in every thread)
                if (tid == f)
                    for (uint32_t b = 0; b < rank; b++) {
                        const Fr9 t = marked(b, tid) ? load_own(b) : fq9_zero();
#pragma unroll
                        for (int i = 0; i < 9; i++) fcol[b * 9u + i] = t.l[i];
                    }
                Fr9 inv = fq9_zero();
                if (pivot) inv = frinv9(load_own(my_row)); // its own pivot value: every pivot thread at once
                __syncthreads();
                if (tid == f) d = fr9_one();
                else if (pivot) d = frmul9(frsub9(fq9_zero(), load_lds(&fcol[my_row * 9u], 1)), inv);
                if (on_pivot) {
                    if (tid == x) {
                        const Fr9 t = frinv9(d);
#pragma unroll
                        for (int i = 0; i < 9; i++) sval[i] = t.l[i];
                    }
                    __syncthreads();
                    d = frmul9(d, load_lds(sval, 1));
                }
            }
            st_fr(&J.emit[tid], fr9_to_standard(d));
        }
    }
}

// ---- what the diagnostics keep on the object (r1cs_obj.h: k16_r1cs::scans).  Ten stages, each made whole by the first call
// that needs it and kept until the object goes; a stage is ready when its pointer is set.
struct ScanList { // the list on the device, and the unbound-wire scan's mask
    DevBuf<uint4>                 inc;     // R1csPair of every incidence of the wires 1 .. n_wires - 1
    DevBuf<uint32_t>              wire;    // their wires
    DevBuf<Fr>                    side;    // merged sums * 2^522 mod r
    DevBuf<unsigned long long>    d_bound; // [ceil(n_wires / 64)]
    PinnedBuf<unsigned long long> h_bound;
};
struct ScanSecond { // the second-value scan
    DevBuf<unsigned long long>    d_kinds; // pinned | rooted, [ceil(n_wires / 64)] each
    PinnedBuf<unsigned long long> h_kinds;
    DevBuf<uint32_t>              d_ref;   // [n_wires] the lowest ROOT incidence of each wire
    DevBuf<uint32_t>              d_list;  // [n_wires] the listed wires
    PinnedBuf<uint32_t>           h_list;
    DevBuf<Fr>                    d_shift; // [n_wires] their shifts, standard form
};
struct ScanDet { // the determinism closure
    DevBuf<uint32_t>              d_start; // [n_wires + 1] the columns of the device list
    DevBuf<unsigned long long>    d_masks; // seed | known, [ceil(n_wires / 64)] each
    PinnedBuf<unsigned long long> h_masks;
    DevBuf<uint32_t>              d_cnt;   // cnt | xr, [M] each
    DevBuf<uint32_t>              d_by;    // by | round, [n_wires] each
    DevBuf<uint32_t>              d_cand, d_front; // [M] / [n_wires]: the two lists
    DevBuf<DetState>              d_state;
    PinnedBuf<DetRecord>          rec;     // pinned, device-mapped
};
struct ScanBool { // the boolean marks: a function of the circuit alone
    R1csBools                  host;
    DevBuf<unsigned long long> d_mark; // [ceil(n_wires / 64)]
};
struct ScanIndex { // the constraint-side index over the device list: by whichever bit rule comes first
    DevBuf<uint32_t> d_cstart; // [M + 1]
    DevBuf<uint32_t> d_cinc;   // [n_pairs]
};
struct ScanHeld { // HELD and the bit rule of the determinism closure
    DevBuf<uint32_t>              d_row;   // the marking rows | the wires they mark, [host.row.size()] each
    DevBuf<unsigned long long>    d_held;  // [ceil(n_wires / 64)]
    PinnedBuf<unsigned long long> h_held;
    DevBuf<uint32_t>              d_bcand; // [M] the bit candidates of a level | [1] their number
    DevBuf<uint8_t>               d_rule;  // [n_wires] K16_DET_RULE_BITS where a bit level derived the wire
};
struct ScanBits { // the bit rule of the witness completion: on top of the completion's stage and the index
    DevBuf<uint8_t>               d_claim;      // [n_pairs] the bit a row claimed for the wire of its incidence
    DevBuf<uint32_t>              d_bcand;      // [M] the bit candidates of a level | [1] their number
    DevBuf<unsigned long long>    d_infeasible; // [n_words] the infeasible rows of the last level
    PinnedBuf<unsigned long long> h_infeasible;
};
struct ScanSolve { // the witness completion: on top of the closure's stage
    DevBuf<uint32_t>              d_rowstart; // [3 M + 1] the row view
    DevBuf<uint2>                 d_term;     // [n_terms]
    DevBuf<Fr>                    d_val;      // [M] a candidate's value, standard form
    DevBuf<unsigned long long>    d_close;    // judged | open, [n_words] each | [1] the flags of k_r1cs_solve_mask | [1] the check's
    PinnedBuf<unsigned long long> h_close;
};
struct ScanOpen { // the open-set solve: every size is bounded by the circuit's, so the buffers are made once
    R1csOpenIndex                 index;     // the constraint-side index over the host list
    R1csOpenWork                  work;      // the work list of the last call
    PinnedBuf<unsigned long long> h_verdict; // [n_words] the check's verdicts
    DevBuf<R1csOpenComp>          d_comp;    // [n_wires]
    DevBuf<uint32_t>              d_rowstart; // [M + 1]
    DevBuf<uint2>                 d_ent;     // [n_pairs]
    DevBuf<unsigned long long>    d_out;     // [3 n_wires] rank | pivot mask | FORCED mask of every component
    PinnedBuf<unsigned long long> h_out;
    DevBuf<uint8_t>               d_cls;     // [n_wires] the classes, by position in the work list's wires
    PinnedBuf<uint8_t>            h_cls;
    DevBuf<Fr>                    d_emit;    // [64] a direction
    PinnedBuf<Fr>                 h_emit;
};
struct ScanOpenWide { // the wide classes of the open-set solve: by the first call with max_wires > 64, beside ScanOpen
    DevBuf<uint32_t>              d_arena;   // OPEN_WIDE_ARENA bytes: the basis slabs of the workgroups of one launch
    DevBuf<unsigned long long>    d_out;     // [9 (n_wires / 65 + 1)] rank | pivot mask [4] | FORCED mask [4] of every wide component
    PinnedBuf<unsigned long long> h_out;
    DevBuf<Fr>                    d_emit;    // [256] a direction
    PinnedBuf<Fr>                 h_emit;
};

} // namespace

struct k16::R1csScans {
    R1csPairs                   pairs; // the host list: by the first call that needs it
    std::unique_ptr<ScanList>   list;
    std::unique_ptr<ScanSecond> second;
    std::unique_ptr<ScanDet>    det;
    std::unique_ptr<ScanSolve>  solve;
    std::unique_ptr<ScanBool>   boolean;
    std::unique_ptr<ScanIndex>  index;
    std::unique_ptr<ScanBits>   bits;
    std::unique_ptr<ScanHeld>   held;
    std::unique_ptr<ScanOpen>   open;
    std::unique_ptr<ScanOpenWide> open_wide;
};
void k16::r1cs_scans_delete(R1csScans* s) { delete s; }

// The incidence list, made once.  K16_ERR_ARG: 2^32 incidences or more.
static int r1cs_pairs_get(k16_ctx* ctx, k16_r1cs* r)
{
    if (r->scans) return K16_OK;
    R1csPlan plan; // the layout k16_r1cs_create_mem uploaded: r1cs_plan_build is a function of the file alone
    if (r1cs_plan_build(r->file, &plan)) {
        ctx->err = "r1cs: too many terms for 32-bit entry offsets";
        return K16_ERR_ARG;
    }
    if (plan.plan.n_entries != r->n_entries) { // positions would point into another layout than d_coef's
        ctx->err = "r1cs: the rebuilt plan is not the one the coefficients were uploaded by";
        return K16_ERR_ARG;
    }
    std::unique_ptr<R1csScans> s(new R1csScans());
    if (r1cs_pairs_build(r->file, plan, &s->pairs)) {
        ctx->err = "r1cs: 2^32 (wire, constraint) incidences or more";
        return K16_ERR_ARG;
    }
    r->scans.reset(s.release());
    return K16_OK;
}

// hipMalloc for the scans: out of device memory is K16_ERR_NOMEM
template <class T>
static int r1cs_scan_alloc(k16_ctx* ctx, DevBuf<T>& b, size_t bytes)
{
    const hipError_t e = b.alloc(std::max<size_t>(bytes, 32));
    if (e == hipSuccess) return K16_OK;
    ctx->err = std::string("r1cs diagnostics: hipMalloc: ") + hipGetErrorString(e);
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? K16_ERR_NOMEM : K16_ERR_HIP;
}

// rc, behind a drain of the stream where it is a failure: nothing of a scan stays in flight
static int r1cs_scan_drained(k16_ctx* ctx, int rc)
{
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

// A stage on first use: built into an owner of its own and installed only when it is whole.  After a failure nothing of it
// remains -- the stream is drained before the owner releases what a copy may still write to -- and a later call starts over.
template <class T, class F>
static int r1cs_scan_stage(k16_ctx* ctx, std::unique_ptr<T>& slot, F&& make)
{
    if (slot) return K16_OK;
    std::unique_ptr<T> fresh(new T());
    const int          rc = r1cs_scan_drained(ctx, make(*fresh));
    if (!rc) slot = std::move(fresh);
    return rc;
}

// what the device list holds: all but wire 0's column, which stays on the host (see k_r1cs_incidences)
static size_t r1cs_walked(const R1csPairs& P) { return P.pair.size() - P.start[1]; }

// list, side table and mask on the device
static int r1cs_scan_upload(k16_ctx* ctx, k16_r1cs* r, ScanList& S)
{
    const R1csPairs&    P    = r->scans->pairs;
    const size_t        skip = P.start[1], n = r1cs_walked(P), words = P.present.size();
    std::vector<R1csFr> side(P.side.size());
    const R1csScale     to_r9(522);
    for (size_t k = 0; k < side.size(); k++) side[k] = to_r9(P.side[k]);
    int rc;
    if ((rc = r1cs_scan_alloc(ctx, S.inc, n * sizeof(R1csPair)))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.wire, n * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.side, side.size() * 32))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_bound, words * 8))) return rc;
    K16_HIP(ctx, S.h_bound.alloc(std::max<size_t>(words * 8, 8)));
    hipStream_t st = ctx->stream;
    if (n) {
        K16_HIP(ctx, hipMemcpyAsync(S.inc, P.pair.data() + skip, n * sizeof(R1csPair), hipMemcpyHostToDevice, st));
        K16_HIP(ctx, hipMemcpyAsync(S.wire, P.wire.data() + skip, n * 4, hipMemcpyHostToDevice, st));
    }
    if (!side.empty()) K16_HIP(ctx, hipMemcpyAsync(S.side, side.data(), side.size() * 32, hipMemcpyHostToDevice, st));
    K16_HIP(ctx, hipStreamSynchronize(st)); // (side is a local)
    return K16_OK;
}

// the host list, the device, the device list
static int r1cs_scan_list(k16_ctx* ctx, k16_r1cs* r)
{
    const int rc = r1cs_pairs_get(ctx, r);
    if (rc) return rc;
    K16_HIP(ctx, hipSetDevice(ctx->device));
    return r1cs_scan_stage(ctx, r->scans->list, [&](ScanList& S) { return r1cs_scan_upload(ctx, r, S); });
}
// What every diagnostic starts with: a completed check to read, and the list.
static int r1cs_scan_checked(k16_ctx* ctx, k16_r1cs* r)
{
    if (!r->have_values || r->forked_on) {
        ctx->err = "no completed check to scan";
        return K16_ERR_ARG;
    }
    return K16_OK;
}
static int r1cs_scan_begin(k16_ctx* ctx, k16_r1cs* r)
{
    const int rc = r1cs_scan_checked(ctx, r);
    return rc ? rc : r1cs_scan_list(ctx, r);
}

// the kernels' view of the device list and of the sums of the last completed check
static IncList r1cs_inc_list(const k16_r1cs* r)
{
    const R1csPairs& P = r->scans->pairs;
    const ScanList&  S = *r->scans->list;
    return IncList{S.inc, S.wire, (uint32_t)r1cs_walked(P), r->d_coef, P.n_entries, S.side, r->d_rows, r->M};
}
static dim3 r1cs_blocks(uint64_t lanes) { return dim3((unsigned)((lanes + 255) / 256)); }

// ---- the unbound-wire scan
static int r1cs_scan_run(k16_ctx* ctx, k16_r1cs* r, const ScanList& S, size_t words)
{
    const IncList L  = r1cs_inc_list(r);
    hipStream_t   st = ctx->stream;
    K16_HIP(ctx, hipMemsetAsync(S.d_bound, 0, words * 8, st));
    if (L.n_pairs) {
        k16_stat_scope sc(ctx, "r1cs_incidences", st);
        hipLaunchKernelGGL(k_r1cs_incidences, r1cs_blocks(L.n_pairs), dim3(256), 0, st, L, S.d_bound);
    }
    K16_HIP(ctx, hipGetLastError());
    K16_HIP(ctx, hipMemcpyAsync(S.h_bound, S.d_bound, words * 8, hipMemcpyDeviceToHost, st));
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
    int      rc  = r1cs_scan_begin(ctx, r);
    if (rc) return rc;
    const std::vector<uint64_t>& present = r->scans->pairs.present;
    const ScanList&              S       = *r->scans->list;
    if ((rc = r1cs_scan_drained(ctx, r1cs_scan_run(ctx, r, S, present.size())))) return rc;
    r1cs_masks_unbound(r->n_wires, present.data(), S.h_bound, n_absent, n_unbound, h_wires, h_class, cap, h_status);
    return K16_OK;
    });
}

// ---- the second-value scan
// masks, references, list and shifts; the incidence list itself is the unbound-wire scan's
static int r1cs_second_alloc(k16_ctx* ctx, k16_r1cs* r, ScanSecond& S)
{
    const size_t words = r->scans->pairs.present.size(), n = r->n_wires;
    int          rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_kinds, 2 * words * 8))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_ref, n * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_list, n * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_shift, n * 32))) return rc;
    K16_HIP(ctx, S.h_kinds.alloc(std::max<size_t>(2 * words * 8, 8)));
    K16_HIP(ctx, S.h_list.alloc(std::max<size_t>(n * 4, 8)));
    return K16_OK;
}

static int r1cs_second_run(k16_ctx* ctx, k16_r1cs* r, uint64_t* n_two_valued, uint32_t* h_wires, uint8_t* h_shift, uint32_t cap,
                           uint8_t* h_status)
{
    const ScanSecond& S     = *r->scans->second;
    const IncList     L     = r1cs_inc_list(r);
    const size_t      words = r->scans->pairs.present.size();
    hipStream_t       st    = ctx->stream;
    K16_HIP(ctx, hipMemsetAsync(S.d_kinds, 0, 2 * words * 8, st));
    K16_HIP(ctx, hipMemsetAsync(S.d_ref, 0xff, (size_t)r->n_wires * 4, st));
    if (L.n_pairs) {
        {
            k16_stat_scope sc(ctx, "r1cs_kinds", st);
            hipLaunchKernelGGL(k_r1cs_kinds, r1cs_blocks(L.n_pairs), dim3(256), 0, st, L, S.d_kinds, S.d_kinds + words, S.d_ref);
        }
        {
            k16_stat_scope sc(ctx, "r1cs_agree", st);
            hipLaunchKernelGGL(k_r1cs_agree, r1cs_blocks(L.n_pairs), dim3(256), 0, st, L, S.d_ref, S.d_kinds);
        }
    }
    K16_HIP(ctx, hipGetLastError());
    K16_HIP(ctx, hipMemcpyAsync(S.h_kinds, S.d_kinds, 2 * words * 8, hipMemcpyDeviceToHost, st));
    K16_HIP(ctx, hipStreamSynchronize(st));
    // the wires are listed for either output: the shifts are those of the listed wires
    const uint32_t listed = r1cs_masks_second(r->n_wires, r->scans->pairs.present.data(), S.h_kinds, S.h_kinds + words, n_two_valued,
                                              h_wires || h_shift ? S.h_list.p : nullptr, cap, h_status);
    if (h_wires && listed) memcpy(h_wires, S.h_list, (size_t)listed * 4);
    if (h_shift && listed) {
        K16_HIP(ctx, hipMemcpyAsync(S.d_list, S.h_list, (size_t)listed * 4, hipMemcpyHostToDevice, st));
        {
            k16_stat_scope sc(ctx, "r1cs_shifts", st);
            hipLaunchKernelGGL(k_r1cs_shifts, dim3((listed + 63) / 64), dim3(64), 0, st, S.d_list, listed, L, S.d_ref, S.d_shift);
        }
        K16_HIP(ctx, hipGetLastError());
        K16_HIP(ctx, hipMemcpyAsync(h_shift, S.d_shift, (size_t)listed * 32, hipMemcpyDeviceToHost, st));
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
    int      rc   = r1cs_scan_begin(ctx, r);
    if (rc) return rc;
    if ((rc = r1cs_scan_stage(ctx, r->scans->second, [&](ScanSecond& S) { return r1cs_second_alloc(ctx, r, S); }))) return rc;
    if ((rc = r1cs_scan_drained(ctx, r1cs_second_run(ctx, r, n_two_valued, h_wires, h_shift, cap, h_status)))) *n_two_valued = 0;
    return rc;
    });
}

// ---- the determinism closure
// column starts, masks, the two words per constraint, the maps and the two lists
static int r1cs_det_alloc(k16_ctx* ctx, k16_r1cs* r, ScanDet& S)
{
    const R1csPairs& P     = r->scans->pairs;
    const size_t     words = P.present.size(), n = r->n_wires, M = r->M;
    int              rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_start, (n + 1) * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_masks, 2 * words * 8))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_cnt, 2 * M * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_by, 2 * n * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_cand, M * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_front, n * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_state, sizeof(DetState)))) return rc;
    K16_HIP(ctx, S.h_masks.alloc(std::max<size_t>(2 * words * 8, 8)));
    K16_HIP(ctx, S.rec.alloc(sizeof(DetRecord), hipHostMallocMapped | hipHostMallocCoherent));
    // the device list leaves wire 0's column out: its columns start that much lower
    const uint32_t        skip = P.start[1];
    std::vector<uint32_t> start(n + 1);
    for (size_t i = 0; i <= n; i++) start[i] = std::max(P.start[i], skip) - skip;
    K16_HIP(ctx, hipMemcpyAsync(S.d_start, start.data(), (n + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    K16_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (start is a local)
    return K16_OK;
}

static dim3 r1cs_capped(uint64_t lanes) { return dim3((unsigned)std::min<uint64_t>((lanes + 255) / 256, DET_GRID)); }

// h_masks[0 .. words) holds the seed: masks, maps, lists and the two words per constraint as round 1 finds them.  Enqueues only.
static int r1cs_det_seed(k16_ctx* ctx, k16_r1cs* r)
{
    const ScanDet&   S     = *r->scans->det;
    const IncList    L     = r1cs_inc_list(r);
    const size_t     words = r->scans->pairs.present.size();
    const uint32_t   M = r->M, n_wires = r->n_wires;
    hipStream_t      st = ctx->stream;
    unsigned long long *d_seed = S.d_masks, *d_known = S.d_masks + words;
    S.rec->n_front = S.rec->n_cand = 0;
    K16_HIP(ctx, hipMemcpyAsync(d_seed, S.h_masks, words * 8, hipMemcpyHostToDevice, st));
    K16_HIP(ctx, hipMemcpyAsync(d_known, S.h_masks, words * 8, hipMemcpyHostToDevice, st));
    K16_HIP(ctx, hipMemsetAsync(S.d_by, 0xff, 2 * (size_t)n_wires * 4, st));
    K16_HIP(ctx, hipMemsetAsync(S.d_state, 0, sizeof(DetState), st));
    if (L.n_pairs && M) {
        K16_HIP(ctx, hipMemsetAsync(S.d_cnt, 0, 2 * (size_t)M * 4, st));
        {
            k16_stat_scope sc(ctx, "r1cs_det_init", st);
            hipLaunchKernelGGL(k_r1cs_det_init, r1cs_blocks(L.n_pairs), dim3(256), 0, st, L, n_wires, d_seed, S.d_cnt, S.d_cnt + M);
            hipLaunchKernelGGL(k_r1cs_det_first, r1cs_capped(M), dim3(256), 0, st, S.d_cnt, M, S.d_cand, S.d_state, S.rec.dev);
        }
        K16_HIP(ctx, hipGetLastError());
    }
    return K16_OK;
}

// Where the rounds stand: cand[0 .. c0) are judged, front[0 .. f0) expanded, `round` levels taken.  A fresh cursor starts behind
// r1cs_det_seed; the witness completion's bit levels move f0 and round on between two runs of the rounds.
struct DetCursor {
    uint32_t c0 = 0, f0 = 0, round = 0;
};

// The rounds behind r1cs_det_seed, one host synchronise each.  derive(c0, c1, f0) enqueues what judges the candidates
// cand[c0 .. c1) of a round and appends the wires they give to front[f0 ..); the expansion follows it here.
template <class Derive>
static int r1cs_det_rounds(k16_ctx* ctx, k16_r1cs* r, DetCursor* cur, Derive&& derive)
{
    const ScanDet&   S     = *r->scans->det;
    const IncList    L     = r1cs_inc_list(r);
    const size_t     words = r->scans->pairs.present.size();
    const uint32_t   M = r->M, n_wires = r->n_wires;
    hipStream_t      st = ctx->stream;
    unsigned long long* d_known = S.d_masks + words;
    uint32_t *          d_cnt = S.d_cnt, *d_xr = S.d_cnt + M, *d_round = S.d_by + n_wires;
    K16_HIP(ctx, hipStreamSynchronize(st));
    // round k judges the candidates [c0, c1) and derives the frontier [f0, f1)
    uint32_t c0 = cur->c0, c1 = S.rec->n_cand, f0 = cur->f0, round = cur->round;
    while (c1 > c0) {
        // every round that goes on adds a wire, and wire 0 is never added: at most n_wires - 1 rounds
        if (round + 1 >= n_wires || c1 > M) {
            ctx->err = "determinism closure: more rounds than wires";
            return K16_ERR_HIP;
        }
        round++;
        const int rc = derive(c0, c1, f0);
        if (rc) return rc;
        {
            // a candidate derives one wire at the most: the frontier is no longer than the candidates' range
            k16_stat_scope sc(ctx, "r1cs_det_expand", st);
            hipLaunchKernelGGL(k_r1cs_det_expand, r1cs_capped(c1 - c0), dim3(256), 0, st, S.d_front, f0, round, S.d_start, L, n_wires,
                               d_known, d_round, d_cnt, d_xr, S.d_cand, S.d_state, S.rec.dev);
        }
        K16_HIP(ctx, hipGetLastError());
        K16_HIP(ctx, hipStreamSynchronize(st));
        const uint32_t f1 = S.rec->n_front, c2 = S.rec->n_cand;
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
    cur->c0 = c1, cur->f0 = f0, cur->round = round; // every candidate listed so far is judged
    return K16_OK;
}

// `known` into h_masks[words ..); round and by as the device left them (r1cs_masks_closure writes round 0 for the seed) where
// asked for.  Enqueues only.
static int r1cs_det_download(k16_ctx* ctx, k16_r1cs* r, uint32_t* h_round, uint32_t* h_by)
{
    const ScanDet& S     = *r->scans->det;
    const size_t   words = r->scans->pairs.present.size();
    const uint32_t n_wires = r->n_wires;
    hipStream_t    st = ctx->stream;
    K16_HIP(ctx, hipMemcpyAsync(S.h_masks + words, S.d_masks + words, words * 8, hipMemcpyDeviceToHost, st));
    if (h_by) K16_HIP(ctx, hipMemcpyAsync(h_by, S.d_by, (size_t)n_wires * 4, hipMemcpyDeviceToHost, st));
    if (h_round) K16_HIP(ctx, hipMemcpyAsync(h_round, S.d_by + n_wires, (size_t)n_wires * 4, hipMemcpyDeviceToHost, st));
    return K16_OK;
}

// The marking rows the last completed check did not find broken, into d_held.  Enqueues only.
static int r1cs_held_enqueue(k16_ctx* ctx, k16_r1cs* r)
{
    const ScanHeld& H     = *r->scans->held;
    const size_t    words = r->scans->pairs.present.size(), rows = r->scans->boolean->host.row.size();
    hipStream_t     st    = ctx->stream;
    K16_HIP(ctx, hipMemsetAsync(H.d_held, 0, std::max<size_t>(words * 8, 8), st));
    if (rows) {
        k16_stat_scope sc(ctx, "r1cs_held", st);
        hipLaunchKernelGGL(k_r1cs_held, r1cs_blocks(rows), dim3(256), 0, st, H.d_row, H.d_row + rows, (uint32_t)rows, r->d_mask, r->M, r->n_wires,
                           H.d_held);
    }
    K16_HIP(ctx, hipGetLastError());
    return K16_OK;
}

// h_masks[0 .. words) holds the seed.  Leaves `known` in h_masks[words ..).  n_by_bits: null for the PIN rule alone; else the
// bit levels are taken (the index, the marks and the held stage are there) and the wires they derived are counted; h_rule then
// gets the device's rule bytes, K16_DET_RULE_BITS where a bit level derived the wire and 0 elsewhere.
static int r1cs_det_run(k16_ctx* ctx, k16_r1cs* r, uint32_t* n_rounds, uint32_t* h_round, uint32_t* h_by, uint64_t* n_by_bits, uint8_t* h_rule)
{
    const ScanDet& S     = *r->scans->det;
    const IncList  L     = r1cs_inc_list(r);
    const size_t   words = r->scans->pairs.present.size();
    const uint32_t M = r->M, n_wires = r->n_wires;
    hipStream_t    st    = ctx->stream;
    int            rc    = r1cs_det_seed(ctx, r);
    if (rc) return rc;
    if (n_by_bits) {
        K16_HIP(ctx, hipMemsetAsync(r->scans->held->d_rule, 0, n_wires, st));
        if ((rc = r1cs_held_enqueue(ctx, r))) return rc;
    }
    DetCursor cur;
    *n_rounds = 0;
    // every bit level that goes on adds a wire, and wire 0 is never added: at most n_wires - 1 of them
    for (uint32_t level = 0;; level++) {
        // the PIN rule to its fixed point
        rc = r1cs_det_rounds(ctx, r, &cur, [&](uint32_t c0, uint32_t c1, uint32_t) {
            k16_stat_scope sc(ctx, "r1cs_det_derive", st);
            hipLaunchKernelGGL(k_r1cs_det_derive, r1cs_blocks(c1 - c0), dim3(256), 0, st, S.d_cand + c0, c1 - c0, L, r->d_mask,
                               S.d_masks + words, S.d_cnt, S.d_cnt + M, n_wires, S.d_by, S.d_front, S.d_state);
            return K16_OK;
        });
        if (rc) return rc;
        // ONE bit level on that state: it is the next round where it derives a wire, and the call's end where it does not
        if (!n_by_bits || !M || !L.n_pairs || cur.round + 1 >= n_wires) break;
        if (level + 1 >= n_wires) {
            ctx->err = "determinism closure: more bit levels than wires";
            return K16_ERR_HIP;
        }
        const ScanHeld&  H       = *r->scans->held;
        const ScanIndex& X       = *r->scans->index;
        uint32_t*        d_total = H.d_bcand + M;
        K16_HIP(ctx, hipMemsetAsync(d_total, 0, 4, st));
        {
            k16_stat_scope sc(ctx, "r1cs_det_bits", st);
            hipLaunchKernelGGL(k_r1cs_bits_filter, r1cs_capped(M), dim3(256), 0, st, S.d_cnt, M, H.d_bcand, d_total);
            hipLaunchKernelGGL(k_r1cs_det_bits, dim3(std::min(M, BITS_GRID)), dim3(64), 0, st, H.d_bcand, d_total, L,
                               RowIndex{X.d_cstart, X.d_cinc}, r->d_mask, S.d_masks + words, H.d_held, S.d_cnt, n_wires, S.d_by, H.d_rule,
                               S.d_front, S.d_state);
        }
        {
            k16_stat_scope sc(ctx, "r1cs_det_expand", st);
            hipLaunchKernelGGL(k_r1cs_det_expand, r1cs_capped(n_wires), dim3(256), 0, st, S.d_front, cur.f0, cur.round + 1, S.d_start, L, n_wires,
                               S.d_masks + words, S.d_by + n_wires, S.d_cnt, S.d_cnt + M, S.d_cand, S.d_state, S.rec.dev);
        }
        K16_HIP(ctx, hipGetLastError());
        K16_HIP(ctx, hipStreamSynchronize(st));
        const uint32_t f1 = S.rec->n_front;
        if (f1 < cur.f0 || f1 > n_wires) {
            ctx->err = "determinism closure: the frontier shrank or outgrew its room";
            return K16_ERR_HIP;
        }
        if (f1 == cur.f0) break; // nothing derived: the fixed point of both rules
        *n_by_bits += f1 - cur.f0;
        cur.round++;
        cur.f0 = f1;
    }
    *n_rounds = cur.round;
    if ((rc = r1cs_det_download(ctx, r, h_round, h_by))) return rc;
    if (n_by_bits && h_rule) K16_HIP(ctx, hipMemcpyAsync(h_rule, r->scans->held->d_rule, n_wires, hipMemcpyDeviceToHost, st));
    K16_HIP(ctx, hipStreamSynchronize(st));
    return K16_OK;
}

// ---- the witness completion
// the row view on the device, the candidates' value slots and the closing pass's masks
static int r1cs_solve_alloc(k16_ctx* ctx, k16_r1cs* r, ScanSolve& S)
{
    R1csPlan plan; // the layout d_coef was uploaded by (see r1cs_pairs_get)
    R1csRows rows;
    if (r1cs_plan_build(r->file, &plan) || plan.plan.n_entries != r->n_entries || r1cs_rows_build(r->file, plan, &rows)) {
        ctx->err = "r1cs: the row view cannot be built (2^32 terms or more, or another plan than the coefficients')";
        return K16_ERR_ARG;
    }
    const size_t words = r->n_words;
    int          rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_rowstart, rows.row_start.size() * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_term, rows.term.size() * sizeof(R1csRowRef)))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_val, (size_t)r->M * 32))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_close, (2 * words + 2) * 8))) return rc;
    K16_HIP(ctx, S.h_close.alloc((2 * words + 2) * 8));
    hipStream_t st = ctx->stream;
    K16_HIP(ctx, hipMemcpyAsync(S.d_rowstart, rows.row_start.data(), rows.row_start.size() * 4, hipMemcpyHostToDevice, st));
    if (!rows.term.empty())
        K16_HIP(ctx, hipMemcpyAsync(S.d_term, rows.term.data(), rows.term.size() * sizeof(R1csRowRef), hipMemcpyHostToDevice, st));
    K16_HIP(ctx, hipStreamSynchronize(st)); // (rows is a local)
    return K16_OK;
}

// the boolean marks, on the host and on the device
static int r1cs_bool_make(k16_ctx* ctx, k16_r1cs* r, ScanBool& S)
{
    r1cs_bools_build(r->file, &S.host);
    const size_t words = S.host.mark.size();
    const int    rc    = r1cs_scan_alloc(ctx, S.d_mark, words * 8);
    if (rc) return rc;
    if (words) K16_HIP(ctx, hipMemcpyAsync(S.d_mark, S.host.mark.data(), words * 8, hipMemcpyHostToDevice, ctx->stream));
    K16_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return K16_OK;
}
static int r1cs_bool_stage(k16_ctx* ctx, k16_r1cs* r)
{
    const int rc = r1cs_pairs_get(ctx, r); // (the owner of every stage)
    if (rc) return rc;
    K16_HIP(ctx, hipSetDevice(ctx->device));
    return r1cs_scan_stage(ctx, r->scans->boolean, [&](ScanBool& S) { return r1cs_bool_make(ctx, r, S); });
}

extern "C" int k16_r1cs_boolean_wires(k16_r1cs* r, uint64_t* n_boolean, uint8_t* h_mark)
{
    return k16_guard(r ? r->ctx : nullptr, [&]() -> int {
    if (!r || !n_boolean) return K16_ERR_ARG;
    *n_boolean   = 0;
    const int rc = r1cs_bool_stage(r->ctx, r);
    if (rc) return rc;
    const R1csBools& B = r->scans->boolean->host;
    *n_boolean         = B.n;
    for (uint32_t i = 0; h_mark && i < r->n_wires; i++) h_mark[i] = (uint8_t)((B.mark[i >> 6] >> (i & 63u)) & 1u);
    return K16_OK;
    });
}

// the constraint-side index over the device list (a counting sort keeps the list's order: by wire)
static int r1cs_index_make(k16_ctx* ctx, k16_r1cs* r, ScanIndex& S)
{
    const R1csPairs&      P    = r->scans->pairs;
    const size_t          skip = P.start[1], n = r1cs_walked(P), M = r->M;
    std::vector<uint32_t> cstart(M + 1, 0), cinc(n);
    for (size_t i = 0; i < n; i++)
        if (P.pair[skip + i].constraint < M) cstart[P.pair[skip + i].constraint + 1]++;
    for (size_t c = 0; c < M; c++) cstart[c + 1] += cstart[c];
    {
        std::vector<uint32_t> cur(cstart.begin(), cstart.end() - 1);
        for (size_t i = 0; i < n; i++)
            if (P.pair[skip + i].constraint < M) cinc[cur[P.pair[skip + i].constraint]++] = (uint32_t)i;
    }
    int rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_cstart, (M + 1) * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_cinc, n * 4))) return rc;
    hipStream_t st = ctx->stream;
    K16_HIP(ctx, hipMemcpyAsync(S.d_cstart, cstart.data(), (M + 1) * 4, hipMemcpyHostToDevice, st));
    if (n) K16_HIP(ctx, hipMemcpyAsync(S.d_cinc, cinc.data(), n * 4, hipMemcpyHostToDevice, st));
    K16_HIP(ctx, hipStreamSynchronize(st)); // (cstart and cinc are locals)
    return K16_OK;
}
static int r1cs_index_stage(k16_ctx* ctx, k16_r1cs* r)
{
    return r1cs_scan_stage(ctx, r->scans->index, [&](ScanIndex& S) { return r1cs_index_make(ctx, r, S); });
}

// the claims, the bit candidates and the infeasible rows of the completion's bit rule
static int r1cs_bits_alloc(k16_ctx* ctx, k16_r1cs* r, ScanBits& S)
{
    const size_t n = r1cs_walked(r->scans->pairs), M = r->M, words = r->n_words;
    int          rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_claim, n))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_bcand, (M + 1) * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_infeasible, words * 8))) return rc;
    K16_HIP(ctx, S.h_infeasible.alloc(std::max<size_t>(words * 8, 8)));
    K16_HIP(ctx, hipMemsetAsync(S.d_claim, 0, std::max<size_t>(n, 1), ctx->stream));
    K16_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return K16_OK;
}

// ---- the determinism closure's entry points, HELD
// the marking rows on the device, the held mask, the closure's bit candidates and rule bytes
static int r1cs_held_alloc(k16_ctx* ctx, k16_r1cs* r, ScanHeld& S)
{
    const R1csBools& B     = r->scans->boolean->host;
    const size_t     words = r->scans->pairs.present.size(), rows = B.row.size();
    int              rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_row, 2 * rows * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_held, words * 8))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_bcand, ((size_t)r->M + 1) * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_rule, r->n_wires))) return rc;
    K16_HIP(ctx, S.h_held.alloc(std::max<size_t>(words * 8, 8)));
    if (rows) { // (B lives as long as the object: the copies read no local)
        K16_HIP(ctx, hipMemcpyAsync(S.d_row, B.row.data(), rows * 4, hipMemcpyHostToDevice, ctx->stream));
        K16_HIP(ctx, hipMemcpyAsync(S.d_row + rows, B.row_wire.data(), rows * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    K16_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return K16_OK;
}
static int r1cs_held_stage(k16_ctx* ctx, k16_r1cs* r)
{
    const int rc = r1cs_bool_stage(ctx, r);
    if (rc) return rc;
    return r1cs_scan_stage(ctx, r->scans->held, [&](ScanHeld& S) { return r1cs_held_alloc(ctx, r, S); });
}

extern "C" int k16_r1cs_held_wires(k16_r1cs* r, uint64_t* n_held, uint8_t* h_mark)
{
    return k16_guard(r ? r->ctx : nullptr, [&]() -> int {
    if (!r || !n_held) return K16_ERR_ARG;
    *n_held      = 0;
    k16_ctx* ctx = r->ctx;
    int      rc  = r1cs_scan_checked(ctx, r);
    if (rc) return rc;
    if ((rc = r1cs_held_stage(ctx, r))) return rc;
    const ScanHeld& H     = *r->scans->held;
    const size_t    words = r->scans->pairs.present.size();
    auto            run   = [&]() -> int {
        const int rc2 = r1cs_held_enqueue(ctx, r);
        if (rc2) return rc2;
        if (words) K16_HIP(ctx, hipMemcpyAsync(H.h_held, H.d_held, words * 8, hipMemcpyDeviceToHost, ctx->stream));
        K16_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return K16_OK;
    };
    if ((rc = r1cs_scan_drained(ctx, run()))) return rc;
    uint64_t n = 0;
    for (size_t w = 0; w < words; w++) n += (uint64_t)__builtin_popcountll(H.h_held[w]);
    *n_held = n;
    for (uint32_t i = 0; h_mark && i < r->n_wires; i++) h_mark[i] = (uint8_t)((H.h_held[i >> 6] >> (i & 63u)) & 1u);
    return K16_OK;
    });
}

// The existing entry point keeps a body of its own, the one it had: its host loops over a seed of a million wires and over the
// masks are a third of a call, and measured 2 to 3 % slower when both entry points shared one function.
extern "C" int k16_r1cs_determined_wires(k16_r1cs* r, const uint32_t* h_seed, uint32_t n_seed, uint64_t* n_derived, uint64_t* n_absent,
                                         uint64_t* n_open, uint32_t* n_rounds, uint32_t* h_wires, uint32_t cap, uint8_t* h_status,
                                         uint32_t* h_round, uint32_t* h_by)
{
    return k16_guard(r ? r->ctx : nullptr, [&]() -> int {
    if (!r || !n_derived || !n_absent || !n_open || !n_rounds || (!h_seed && n_seed)) return K16_ERR_ARG;
    *n_derived = *n_absent = *n_open = 0;
    *n_rounds                        = 0;
    k16_ctx* ctx                     = r->ctx;
    int      rc                      = r1cs_scan_begin(ctx, r);
    if (rc) return rc;
    if ((rc = r1cs_scan_stage(ctx, r->scans->det, [&](ScanDet& S) { return r1cs_det_alloc(ctx, r, S); }))) return rc;
    const ScanDet& S     = *r->scans->det;
    const size_t   words = r->scans->pairs.present.size();
    if (const char* why = r1cs_seed_mask(r->n_wires, r->file.n_pub_out, r->file.n_pub_in, r->file.n_prv_in, h_seed, n_seed, S.h_masks)) {
        ctx->err = why;
        return K16_ERR_ARG;
    }
    if ((rc = r1cs_scan_drained(ctx, r1cs_det_run(ctx, r, n_rounds, h_round, h_by, nullptr, nullptr)))) {
        *n_rounds = 0;
        return rc;
    }
    const uint64_t* present = r->scans->pairs.present.data();
    r1cs_masks_closure(r->n_wires, present, S.h_masks, S.h_masks + words, n_derived, n_absent, n_open, h_wires, cap, h_status, h_round);
    return K16_OK;
    });
}

// The same call with `rules`; K16_DET_RULE_PIN takes the same path through r1cs_det_run.
extern "C" int k16_r1cs_determined_wires_ex(k16_r1cs* r, const uint32_t* h_seed, uint32_t n_seed, uint32_t rules, uint64_t* n_derived,
                                            uint64_t* n_absent, uint64_t* n_open, uint32_t* n_rounds, uint32_t* h_wires, uint32_t cap,
                                            uint8_t* h_status, uint32_t* h_round, uint32_t* h_by, uint64_t* n_by_bits, uint8_t* h_rule)
{
    return k16_guard(r ? r->ctx : nullptr, [&]() -> int {
    if (!r || !n_derived || !n_absent || !n_open || !n_rounds || !n_by_bits || (!h_seed && n_seed)) return K16_ERR_ARG;
    *n_derived = *n_absent = *n_open = *n_by_bits = 0;
    *n_rounds                                    = 0;
    k16_ctx* ctx                                 = r->ctx;
    if (rules != K16_DET_RULE_PIN && rules != (K16_DET_RULE_PIN | K16_DET_RULE_BITS)) {
        ctx->err = "determinism closure: rules is neither K16_DET_RULE_PIN nor K16_DET_RULE_PIN | K16_DET_RULE_BITS";
        return K16_ERR_ARG;
    }
    const bool with_bits = (rules & K16_DET_RULE_BITS) != 0;
    int        rc        = r1cs_scan_begin(ctx, r);
    if (rc) return rc;
    if ((rc = r1cs_scan_stage(ctx, r->scans->det, [&](ScanDet& S) { return r1cs_det_alloc(ctx, r, S); }))) return rc;
    const ScanDet& S     = *r->scans->det;
    const size_t   words = r->scans->pairs.present.size();
    if (const char* why = r1cs_seed_mask(r->n_wires, r->file.n_pub_out, r->file.n_pub_in, r->file.n_prv_in, h_seed, n_seed, S.h_masks)) {
        ctx->err = why;
        return K16_ERR_ARG;
    }
    if (with_bits) {
        if ((rc = r1cs_held_stage(ctx, r))) return rc;
        if ((rc = r1cs_index_stage(ctx, r))) return rc;
    }
    if ((rc = r1cs_scan_drained(ctx, r1cs_det_run(ctx, r, n_rounds, h_round, h_by, with_bits ? n_by_bits : nullptr, h_rule)))) {
        *n_rounds = 0;
        *n_by_bits = 0;
        return rc;
    }
    const uint64_t* present = r->scans->pairs.present.data();
    r1cs_masks_closure(r->n_wires, present, S.h_masks, S.h_masks + words, n_derived, n_absent, n_open, h_wires, cap, h_status, h_round);
    if (h_rule) { // a derived wire that no bit level wrote is the PIN rule's
        const unsigned long long *seed = S.h_masks, *known = S.h_masks + words;
        for (uint32_t i = 0; i < r->n_wires; i++) {
            const bool derived = ((known[i >> 6] & ~seed[i >> 6]) >> (i & 63u)) & 1ull;
            h_rule[i] = !derived ? 0 : with_bits && h_rule[i] == K16_DET_RULE_BITS ? K16_DET_RULE_BITS : K16_DET_RULE_PIN;
        }
    }
    return K16_OK;
    });
}

// what the bit levels of a run did, for the host's maps
struct BitsRun {
    uint64_t              n_by_bits = 0;
    std::vector<uint32_t> rounds; // the rounds that were bit levels, ascending
};

// h_masks[0 .. words) of the closure's stage holds the givens.  K16_ERR_FORMAT before any round when a given value is refused;
// else leaves the completed assignment in d_wtns and h_wtns, its check in d_rows / d_mask, `known` in h_masks[words ..), and
// judged | open in h_close.  bits: null for the linear rule alone; else the bit levels are taken and the infeasible rows of the
// final state lie in the bit stage's h_infeasible.
static int r1cs_solve_run(k16_ctx* ctx, k16_r1cs* r, void* h_wtns, uint32_t* n_rounds, uint32_t* h_round, uint32_t* h_by, BitsRun* bits)
{
    const ScanDet&   S     = *r->scans->det;
    const ScanSolve& V     = *r->scans->solve;
    const IncList    L     = r1cs_inc_list(r);
    const RowView    rows  = {V.d_rowstart, V.d_term};
    const size_t     words = r->scans->pairs.present.size(), cw = r->n_words;
    const uint32_t   M = r->M, n_wires = r->n_wires;
    hipStream_t      st = ctx->stream;
    unsigned long long* d_flags = V.d_close + 2 * cw;
    int                 rc;
    V.h_close[2 * cw] = V.h_close[2 * cw + 1] = ~0ull;
    K16_HIP(ctx, hipMemcpyAsync(r->d_wtns, h_wtns, (size_t)n_wires * 32, hipMemcpyHostToDevice, st));
    K16_HIP(ctx, hipMemsetAsync(d_flags, 0, 8, st));
    if ((rc = r1cs_det_seed(ctx, r))) return rc;
    {
        k16_stat_scope sc(ctx, "r1cs_solve_mask", st);
        hipLaunchKernelGGL(k_r1cs_solve_mask, r1cs_blocks(n_wires), dim3(256), 0, st, (uint4*)r->d_wtns.p, n_wires, S.d_masks, d_flags);
    }
    K16_HIP(ctx, hipGetLastError());
    K16_HIP(ctx, hipMemcpyAsync(V.h_close + 2 * cw, d_flags, 8, hipMemcpyDeviceToHost, st));
    K16_HIP(ctx, hipStreamSynchronize(st));
    if (const unsigned long long flags = V.h_close[2 * cw]) {
        ctx->err = (flags & WTNS_NOT_BELOW_R) ? "witness: a given wire's value is not below r" : "witness: wire 0 is not 1";
        return K16_ERR_FORMAT;
    }
    DetCursor cur;
    *n_rounds = 0;
    // for the run that takes no bit level at all (no constraints, no incidences): the mask is downloaded whatever happened.
    // Every level clears it again, so that what is reported is the last level's
    if (bits) K16_HIP(ctx, hipMemsetAsync(r->scans->bits->d_infeasible, 0, std::max<size_t>(cw * 8, 8), st));
    for (;;) {
        // the linear rule to its fixed point
        rc = r1cs_det_rounds(ctx, r, &cur, [&](uint32_t c0, uint32_t c1, uint32_t f0) {
            {
                k16_stat_scope sc(ctx, "r1cs_solve_derive", st);
                hipLaunchKernelGGL(k_r1cs_solve_derive, r1cs_blocks(c1 - c0), dim3(256), 0, st, S.d_cand + c0, c1 - c0, L, rows, r->d_wtns,
                                   S.d_masks + words, S.d_cnt, S.d_cnt + M, n_wires, S.d_by, V.d_val, S.d_front, S.d_state);
            }
            k16_stat_scope sc(ctx, "r1cs_solve_commit", st);
            hipLaunchKernelGGL(k_r1cs_solve_commit, r1cs_capped(c1 - c0), dim3(256), 0, st, S.d_front, f0, S.d_state, S.d_by, V.d_val,
                               n_wires, M, r->d_wtns);
            return K16_OK;
        });
        if (rc) return rc;
        // ONE bit level on that state: it is the next round where it solves a wire, and the call's end where it does not
        if (!bits || !M || !L.n_pairs || cur.round + 1 >= n_wires) break;
        const ScanBits& B       = *r->scans->bits;
        uint32_t*       d_total = B.d_bcand + M;
        K16_HIP(ctx, hipMemsetAsync(d_total, 0, 4, st));
        K16_HIP(ctx, hipMemsetAsync(B.d_infeasible, 0, cw * 8, st)); // what is reported is the LAST level's: the final state's
        {
            k16_stat_scope sc(ctx, "r1cs_solve_bits", st);
            hipLaunchKernelGGL(k_r1cs_bits_filter, r1cs_capped(M), dim3(256), 0, st, S.d_cnt, M, B.d_bcand, d_total);
            hipLaunchKernelGGL(k_r1cs_solve_bits, dim3(std::min(M, BITS_GRID)), dim3(64), 0, st, B.d_bcand, d_total, L, rows,
                               RowIndex{r->scans->index->d_cstart, r->scans->index->d_cinc}, r->d_wtns, S.d_masks + words, r->scans->boolean->d_mark, S.d_cnt, n_wires, S.d_by,
                               B.d_claim, B.d_infeasible, S.d_front, S.d_state);
            hipLaunchKernelGGL(k_r1cs_bits_commit, r1cs_capped(n_wires), dim3(256), 0, st, S.d_front, cur.f0, S.d_state, S.d_by, S.d_start, L,
                               B.d_claim, n_wires, (uint4*)r->d_wtns.p);
        }
        {
            k16_stat_scope sc(ctx, "r1cs_det_expand", st);
            hipLaunchKernelGGL(k_r1cs_det_expand, r1cs_capped(n_wires), dim3(256), 0, st, S.d_front, cur.f0, cur.round + 1, S.d_start, L, n_wires,
                               S.d_masks + words, S.d_by + n_wires, S.d_cnt, S.d_cnt + M, S.d_cand, S.d_state, S.rec.dev);
        }
        K16_HIP(ctx, hipGetLastError());
        K16_HIP(ctx, hipStreamSynchronize(st));
        const uint32_t f1 = S.rec->n_front;
        if (f1 < cur.f0 || f1 > n_wires) {
            ctx->err = "witness completion: the frontier shrank or outgrew its room";
            return K16_ERR_HIP;
        }
        if (f1 == cur.f0) break; // nothing solved: the state the infeasible rows were found in is final
        bits->n_by_bits += f1 - cur.f0;
        bits->rounds.push_back(++cur.round);
        cur.f0 = f1;
    }
    *n_rounds = cur.round;
    // the closing pass: the check's own kernels on the completed assignment, then the open constraints' verdicts taken out
    if ((rc = k16_r1cs_launch(r, st, r->d_wtns))) return rc;
    if (M) {
        if (!L.n_pairs) K16_HIP(ctx, hipMemsetAsync(S.d_cnt, 0, (size_t)M * 4, st)); // (r1cs_det_seed had nothing to count)
        k16_stat_scope sc(ctx, "r1cs_solve_close", st);
        hipLaunchKernelGGL(k_r1cs_solve_close, r1cs_blocks(M), dim3(256), 0, st, r->d_mask, S.d_cnt, M, r->n_words, V.d_close, V.d_close + cw);
    }
    K16_HIP(ctx, hipGetLastError());
    K16_HIP(ctx, hipMemcpyAsync(V.d_close + 2 * cw + 1, r->d_mask + cw, 8, hipMemcpyDeviceToDevice, st));
    K16_HIP(ctx, hipMemcpyAsync(V.h_close, V.d_close, (2 * cw + 2) * 8, hipMemcpyDeviceToHost, st));
    if (bits && cw) K16_HIP(ctx, hipMemcpyAsync(r->scans->bits->h_infeasible, r->scans->bits->d_infeasible, cw * 8, hipMemcpyDeviceToHost, st));
    if ((rc = r1cs_det_download(ctx, r, h_round, h_by))) return rc;
    K16_HIP(ctx, hipStreamSynchronize(st));
    if (V.h_close[2 * cw + 1]) { // every value on the device is canonical by now and wire 0 was found to be 1
        ctx->err = "witness completion: the closing check refused the completed assignment";
        return K16_ERR_HIP;
    }
    K16_HIP(ctx, hipMemcpyAsync(h_wtns, r->d_wtns, (size_t)n_wires * 32, hipMemcpyDeviceToHost, st));
    K16_HIP(ctx, hipStreamSynchronize(st));
    return K16_OK;
}

// what k16_r1cs_complete_witness_ex returns beyond k16_r1cs_complete_witness
struct BitsOut {
    uint64_t *n_by_bits, *n_infeasible;
    uint32_t* h_infeasible;
    uint32_t  cap_infeasible;
    uint8_t*  h_rule;
};

// both entry points; ex: null for k16_r1cs_complete_witness
static int r1cs_complete(k16_r1cs* r, void* h_wtns, const uint32_t* h_given, uint32_t n_given, uint32_t rules, uint64_t* n_solved,
                         uint64_t* n_absent, uint64_t* n_open, uint32_t* n_rounds, uint64_t* n_failed, uint32_t* h_failed, uint32_t cap_failed,
                         uint64_t* n_open_constraints, uint32_t* h_wires, uint32_t cap, uint8_t* h_status, uint32_t* h_round, uint32_t* h_by,
                         const BitsOut* ex)
{
    if (!r || !h_wtns || !n_solved || !n_absent || !n_open || !n_rounds || !n_failed || !n_open_constraints || (!h_given && n_given))
        return K16_ERR_ARG;
    if (ex && (!ex->n_by_bits || !ex->n_infeasible)) return K16_ERR_ARG;
    *n_solved = *n_absent = *n_open = *n_failed = *n_open_constraints = 0;
    *n_rounds                                                        = 0;
    if (ex) *ex->n_by_bits = *ex->n_infeasible = 0;
    k16_ctx* ctx = r->ctx;
    if (rules != K16_SOLVE_RULE_LINEAR && rules != (K16_SOLVE_RULE_LINEAR | K16_SOLVE_RULE_BITS)) {
        ctx->err = "witness completion: rules is neither K16_SOLVE_RULE_LINEAR nor K16_SOLVE_RULE_LINEAR | K16_SOLVE_RULE_BITS";
        return K16_ERR_ARG;
    }
    if (r->forked_on) {
        ctx->err = "witness completion: a prove call is running on the object";
        return K16_ERR_ARG;
    }
    r->have_values = false; // from here on the sums are this call's, or nobody's: an error leaves no completed check
    // the givens are looked at before anything is built or launched
    if (!h_given && (uint64_t)r->file.n_pub_out + 1 + r->file.n_pub_in + r->file.n_prv_in > r->n_wires) {
        ctx->err = "the header's input wires reach beyond nWires";
        return K16_ERR_ARG;
    }
    for (uint32_t k = 0; h_given && k < n_given; k++) {
        if (h_given[k] >= r->n_wires) {
            ctx->err = "given wire number out of range";
            return K16_ERR_ARG;
        }
    }
    const bool with_bits = (rules & K16_SOLVE_RULE_BITS) != 0;
    int        rc        = r1cs_scan_list(ctx, r);
    if (rc) return rc;
    if ((rc = r1cs_scan_stage(ctx, r->scans->det, [&](ScanDet& S) { return r1cs_det_alloc(ctx, r, S); }))) return rc;
    if ((rc = r1cs_scan_stage(ctx, r->scans->solve, [&](ScanSolve& S) { return r1cs_solve_alloc(ctx, r, S); }))) return rc;
    if (with_bits) {
        if ((rc = r1cs_bool_stage(ctx, r))) return rc;
        if ((rc = r1cs_index_stage(ctx, r))) return rc;
        if ((rc = r1cs_scan_stage(ctx, r->scans->bits, [&](ScanBits& S) { return r1cs_bits_alloc(ctx, r, S); }))) return rc;
    }
    const ScanDet&   S     = *r->scans->det;
    const ScanSolve& V     = *r->scans->solve;
    const size_t     words = r->scans->pairs.present.size(), cw = r->n_words;
    if (const char* why = r1cs_seed_mask(r->n_wires, r->file.n_pub_out, r->file.n_pub_in, r->file.n_prv_in, h_given, n_given, S.h_masks)) {
        ctx->err = why;
        return K16_ERR_ARG;
    }
    // the rule of a wire is its round's: the rounds are needed for h_rule whether the caller asked for them or not
    BitsRun               run;
    std::vector<uint32_t> own_round;
    uint32_t*             rounds = h_round;
    if (ex && ex->h_rule && !h_round && with_bits) {
        own_round.resize(r->n_wires);
        rounds = own_round.data();
    }
    if ((rc = r1cs_scan_drained(ctx, r1cs_solve_run(ctx, r, h_wtns, n_rounds, rounds, h_by, with_bits ? &run : nullptr)))) {
        *n_rounds = 0;
        return rc;
    }
    r->have_values = true;
    r1cs_masks_closure(r->n_wires, r->scans->pairs.present.data(), S.h_masks, S.h_masks + words, n_solved, n_absent, n_open, h_wires, cap,
                       h_status, h_round);
    uint64_t failed = 0, open = 0;
    for (size_t w = 0; w < cw; w++) {
        open += (uint64_t)__builtin_popcountll(V.h_close[cw + w]);
        for (unsigned long long m = V.h_close[w]; m; m &= m - 1, failed++)
            if (h_failed && failed < cap_failed) h_failed[failed] = (uint32_t)(w * 64u) + (uint32_t)__builtin_ctzll(m);
    }
    *n_failed = failed, *n_open_constraints = open;
    if (!ex) return K16_OK;
    *ex->n_by_bits = run.n_by_bits;
    if (with_bits) {
        const unsigned long long* inf   = r->scans->bits->h_infeasible;
        uint64_t                  count = 0, listed = 0;
        for (size_t w = 0; w < cw; w++) {
            count += (uint64_t)__builtin_popcountll(inf[w]);
            if (ex->h_infeasible) listed = r1cs_mask_list(w, inf[w], listed, ex->cap_infeasible, ex->h_infeasible);
        }
        *ex->n_infeasible = count;
    }
    if (ex->h_rule) {
        const unsigned long long *seed = S.h_masks, *known = S.h_masks + words;
        for (uint32_t i = 0; i < r->n_wires; i++) {
            const bool solved = ((known[i >> 6] & ~seed[i >> 6]) >> (i & 63u)) & 1ull;
            ex->h_rule[i]     = !solved ? 0 : with_bits && std::binary_search(run.rounds.begin(), run.rounds.end(), rounds[i]) ? 2 : 1;
        }
    }
    return K16_OK;
}

extern "C" int k16_r1cs_complete_witness(k16_r1cs* r, void* h_wtns, const uint32_t* h_given, uint32_t n_given, uint64_t* n_solved,
                                         uint64_t* n_absent, uint64_t* n_open, uint32_t* n_rounds, uint64_t* n_failed, uint32_t* h_failed,
                                         uint32_t cap_failed, uint64_t* n_open_constraints, uint32_t* h_wires, uint32_t cap, uint8_t* h_status,
                                         uint32_t* h_round, uint32_t* h_by)
{
    return k16_guard(r ? r->ctx : nullptr, [&]() -> int {
    return r1cs_complete(r, h_wtns, h_given, n_given, K16_SOLVE_RULE_LINEAR, n_solved, n_absent, n_open, n_rounds, n_failed, h_failed, cap_failed,
                         n_open_constraints, h_wires, cap, h_status, h_round, h_by, nullptr);
    });
}

extern "C" int k16_r1cs_complete_witness_ex(k16_r1cs* r, void* h_wtns, const uint32_t* h_given, uint32_t n_given, uint32_t rules,
                                            uint64_t* n_solved, uint64_t* n_absent, uint64_t* n_open, uint32_t* n_rounds, uint64_t* n_failed,
                                            uint32_t* h_failed, uint32_t cap_failed, uint64_t* n_open_constraints, uint32_t* h_wires, uint32_t cap,
                                            uint8_t* h_status, uint32_t* h_round, uint32_t* h_by, uint64_t* n_by_bits, uint64_t* n_infeasible,
                                            uint32_t* h_infeasible, uint32_t cap_infeasible, uint8_t* h_rule)
{
    return k16_guard(r ? r->ctx : nullptr, [&]() -> int {
    const BitsOut ex = {n_by_bits, n_infeasible, h_infeasible, cap_infeasible, h_rule};
    return r1cs_complete(r, h_wtns, h_given, n_given, rules, n_solved, n_absent, n_open, n_rounds, n_failed, h_failed, cap_failed,
                         n_open_constraints, h_wires, cap, h_status, h_round, h_by, &ex);
    });
}

// ---- the open-set solve
constexpr uint32_t OPEN_GRID = 4096; // workgroups (of one wave) of a launch of k_r1cs_open_rref: a workgroup strides the components

// the constraint-side index on the host and every buffer: their sizes are bounded by the circuit's (a component has a wire, a
// row is a constraint, an entry an incidence), so one allocation serves every mask
static int r1cs_open_alloc(k16_ctx* ctx, k16_r1cs* r, ScanOpen& S)
{
    const R1csPairs& P = r->scans->pairs;
    const size_t     n = r->n_wires, M = r->M, np = r1cs_walked(P), words = r->n_words;
    r1cs_open_index(P, r->M, &S.index);
    int rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_comp, n * sizeof(R1csOpenComp)))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_rowstart, (M + 1) * 4))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_ent, np * sizeof(uint2)))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_out, 3 * n * 8))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_cls, n))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_emit, 64 * sizeof(Fr)))) return rc;
    K16_HIP(ctx, S.h_verdict.alloc(std::max<size_t>(words * 8, 8)));
    K16_HIP(ctx, S.h_out.alloc(std::max<size_t>(3 * n * 8, 8)));
    K16_HIP(ctx, S.h_cls.alloc(std::max<size_t>(n, 8)));
    K16_HIP(ctx, S.h_emit.alloc(64 * sizeof(Fr)));
    return K16_OK;
}

// What both entry points start with: a completed check, the list, the stage, the fixed mask and the check's verdicts on the host.
static int r1cs_open_begin(k16_ctx* ctx, k16_r1cs* r, const uint8_t* h_fixed)
{
    int rc = r1cs_scan_checked(ctx, r);
    if (rc) return rc;
    if (!h_fixed) {
        ctx->err = "open-set solve: no mask of fixed wires";
        return K16_ERR_ARG;
    }
    if ((rc = r1cs_scan_list(ctx, r))) return rc;
    if ((rc = r1cs_scan_stage(ctx, r->scans->open, [&](ScanOpen& S) { return r1cs_open_alloc(ctx, r, S); }))) return rc;
    const ScanOpen& S = *r->scans->open;
    memset(S.h_verdict, 0, std::max<size_t>((size_t)r->n_words * 8, 8));
    auto get = [&]() -> int {
        if (r->n_words) K16_HIP(ctx, hipMemcpyAsync(S.h_verdict, r->d_mask, (size_t)r->n_words * 8, hipMemcpyDeviceToHost, ctx->stream));
        K16_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return K16_OK;
    };
    return r1cs_scan_drained(ctx, get());
}

template <uint32_t W>
static void r1cs_open_launch(k16_ctx* ctx, const char* name, const IncList& L, OpenJob J, uint32_t first, uint32_t n)
{
    if (!n) return;
    J.comp += first;
    J.out += 3 * (size_t)first;
    J.n_comp = n;
    k16_stat_scope sc(ctx, name, ctx->stream);
    hipLaunchKernelGGL(k_r1cs_open_rref<W>, dim3(std::min(n, OPEN_GRID)), dim3(64), 0, ctx->stream, L, J);
}

// The wide classes.  One arena of basis slabs, shared by both (their launches follow each other on the stream): 144 MiB =
// 256 slabs of 128 x 9 x 128 words (0.5625 MiB: one workgroup of 2 waves on each of the chip's 256 CUs) = 64 slabs of
// 256 x 9 x 256 words (2.25 MiB: one workgroup of 4 waves on a quarter of the CUs).  The grid of a launch never passes the
// slabs: a workgroup strides the components of its class.
constexpr size_t OPEN_WIDE_ARENA = (size_t)144 << 20;
template <uint32_t W>
constexpr uint32_t open_wide_grid() { return (uint32_t)(OPEN_WIDE_ARENA / ((size_t)W * 9 * W * 4)); }
static_assert(open_wide_grid<128>() == 256 && open_wide_grid<256>() == 64, "the arena is cut into whole slabs");

static int r1cs_open_wide_alloc(k16_ctx* ctx, k16_r1cs* r, ScanOpenWide& S)
{
    const size_t n_out = 9 * ((size_t)r->n_wires / (R1CS_OPEN_MAX_WIRES + 1) + 1) * 8;
    int          rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_arena, OPEN_WIDE_ARENA))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_out, n_out))) return rc;
    if ((rc = r1cs_scan_alloc(ctx, S.d_emit, R1CS_OPEN_MAX_WIRES_EX * sizeof(Fr)))) return rc;
    K16_HIP(ctx, S.h_out.alloc(n_out));
    K16_HIP(ctx, S.h_emit.alloc(R1CS_OPEN_MAX_WIRES_EX * sizeof(Fr)));
    return K16_OK;
}

template <uint32_t W>
static void r1cs_open_launch_wide(k16_ctx* ctx, const char* name, const IncList& L, OpenJob J, const ScanOpenWide& Sw, uint32_t first,
                                  uint32_t first_wide, uint32_t n)
{
    if (!n) return;
    J.comp += first;
    J.out = Sw.d_out.p + 9 * (size_t)first_wide;
    J.n_comp = n;
    if (J.emit) J.emit = Sw.d_emit.p;
    k16_stat_scope sc(ctx, name, ctx->stream);
    hipLaunchKernelGGL(k_r1cs_open_rref_wide<W>, dim3(std::min(n, open_wide_grid<W>())), dim3(W), 0, ctx->stream, L, J, Sw.d_arena.p);
}

// What the last run left for component k of the work list: its rank, and the direction the emit path wrote.
static uint64_t r1cs_open_rank(const k16_r1cs* r, size_t k)
{
    const R1csOpenWork& Wk     = r->scans->open->work;
    const size_t        narrow = (size_t)Wk.n_class[0] + Wk.n_class[1] + Wk.n_class[2];
    return k < narrow ? r->scans->open->h_out[3 * k] : r->scans->open_wide->h_out[9 * (k - narrow)];
}

// The work list up, one launch per size class, ranks, masks and classes (and the direction of column emit_col, where asked) down.
// The wide classes are empty unless the list was built with a cap above R1CS_OPEN_MAX_WIRES, and then the wide stage is there.
static int r1cs_open_run(k16_ctx* ctx, k16_r1cs* r, bool emit, uint32_t emit_col)
{
    const ScanOpen&     S  = *r->scans->open;
    const R1csOpenWork& Wk = S.work;
    const size_t        nc = Wk.comps.size(), nw = Wk.wires.size(), nr = Wk.row.size(), ne = Wk.ent.size();
    if (!nc) return K16_OK;
    const uint32_t narrow = Wk.n_class[0] + Wk.n_class[1] + Wk.n_class[2], wide = Wk.n_class[3] + Wk.n_class[4];
    if (nc > r->n_wires || nw > r->n_wires || nr > r->M || ne > r1cs_walked(r->scans->pairs) || (size_t)narrow + wide != nc ||
        (wide && (!r->scans->open_wide || wide > r->n_wires / (R1CS_OPEN_MAX_WIRES + 1)))) {
        ctx->err = "open-set solve: the work list outgrew the circuit";
        return K16_ERR_HIP;
    }
    hipStream_t st = ctx->stream;
    {
        k16_stat_scope sc(ctx, "r1cs_open_upload", st);
        K16_HIP(ctx, hipMemcpyAsync(S.d_comp, Wk.comps.data(), nc * sizeof(R1csOpenComp), hipMemcpyHostToDevice, st));
        K16_HIP(ctx, hipMemcpyAsync(S.d_rowstart, Wk.row_start.data(), (nr + 1) * 4, hipMemcpyHostToDevice, st));
        if (ne) K16_HIP(ctx, hipMemcpyAsync(S.d_ent, Wk.ent.data(), ne * sizeof(R1csOpenEntry), hipMemcpyHostToDevice, st));
        K16_HIP(ctx, hipMemsetAsync(S.d_cls, 0xff, nw, st));
    }
    const IncList L = r1cs_inc_list(r);
    const OpenJob J{S.d_comp, 0, S.d_rowstart, S.d_ent, (uint32_t)nr, (uint32_t)ne, (uint32_t)nw, S.d_out, S.d_cls, emit ? S.d_emit.p : nullptr, emit_col};
    r1cs_open_launch<16>(ctx, "r1cs_open_rref16", L, J, 0, Wk.n_class[0]);
    r1cs_open_launch<32>(ctx, "r1cs_open_rref32", L, J, Wk.n_class[0], Wk.n_class[1]);
    r1cs_open_launch<64>(ctx, "r1cs_open_rref64", L, J, Wk.n_class[0] + Wk.n_class[1], Wk.n_class[2]);
    if (wide) {
        const ScanOpenWide& Sw = *r->scans->open_wide;
        r1cs_open_launch_wide<128>(ctx, "r1cs_open_rref128", L, J, Sw, narrow, 0, Wk.n_class[3]);
        r1cs_open_launch_wide<256>(ctx, "r1cs_open_rref256", L, J, Sw, narrow + Wk.n_class[3], Wk.n_class[3], Wk.n_class[4]);
    }
    K16_HIP(ctx, hipGetLastError());
    if (narrow) K16_HIP(ctx, hipMemcpyAsync(S.h_out, S.d_out, 3 * (size_t)narrow * 8, hipMemcpyDeviceToHost, st));
    K16_HIP(ctx, hipMemcpyAsync(S.h_cls, S.d_cls, nw, hipMemcpyDeviceToHost, st));
    if (emit && narrow) K16_HIP(ctx, hipMemcpyAsync(S.h_emit, S.d_emit, 64 * sizeof(Fr), hipMemcpyDeviceToHost, st));
    if (wide) {
        const ScanOpenWide& Sw = *r->scans->open_wide;
        K16_HIP(ctx, hipMemcpyAsync(Sw.h_out, Sw.d_out, 9 * (size_t)wide * 8, hipMemcpyDeviceToHost, st));
        if (emit) K16_HIP(ctx, hipMemcpyAsync(Sw.h_emit, Sw.d_emit, R1CS_OPEN_MAX_WIRES_EX * sizeof(Fr), hipMemcpyDeviceToHost, st));
    }
    K16_HIP(ctx, hipStreamSynchronize(st));
    for (size_t k = 0; k < nw; k++)
        if (S.h_cls[k] != K16_OPEN_FORCED && S.h_cls[k] != K16_OPEN_FREE && S.h_cls[k] != K16_OPEN_UNDECIDED) {
            ctx->err = "open-set solve: the kernel left a wire without a class";
            return K16_ERR_HIP;
        }
    return K16_OK;
}

// The cap of an _ex call, judged before anything is launched or written.
static int r1cs_open_cap(k16_ctx* ctx, uint32_t max_wires)
{
    if (max_wires < R1CS_OPEN_MAX_WIRES || max_wires > R1CS_OPEN_MAX_WIRES_EX) {
        ctx->err = "open-set solve: max_wires outside 64 .. 256";
        return K16_ERR_ARG;
    }
    return K16_OK;
}
// The wide stage, where the cap asks for it: made by the first such call.
static int r1cs_open_wide_stage(k16_ctx* ctx, k16_r1cs* r, uint32_t max_wires)
{
    if (max_wires <= R1CS_OPEN_MAX_WIRES) return K16_OK;
    return r1cs_scan_stage(ctx, r->scans->open_wide, [&](ScanOpenWide& S) { return r1cs_open_wide_alloc(ctx, r, S); });
}

static int r1cs_open_system(k16_r1cs* r, const uint8_t* h_fixed, uint32_t max_wires, uint64_t* n_forced, uint64_t* n_free,
                            uint64_t* n_undecided, uint64_t* n_skipped, uint64_t* n_absent, uint64_t* n_components, uint64_t* n_dims,
                            uint32_t* h_wires, uint8_t* h_class, uint32_t cap, uint8_t* h_status, uint32_t* h_comp)
{
    *n_forced = *n_free = *n_undecided = *n_skipped = *n_absent = *n_components = *n_dims = 0;
    k16_ctx* ctx = r->ctx;
    int      rc  = r1cs_open_begin(ctx, r, h_fixed);
    if (rc) return rc;
    if ((rc = r1cs_open_wide_stage(ctx, r, max_wires))) return rc;
    ScanOpen& S = *r->scans->open;
    r1cs_open_build(r->scans->pairs, S.index, r->n_wires, r->M, h_fixed, (const uint64_t*)S.h_verdict.p, &S.work, max_wires);
    if ((rc = r1cs_scan_drained(ctx, r1cs_open_run(ctx, r, false, 0)))) return rc;
    R1csOpenWork& Wk = S.work;
    uint64_t      dims = 0;
    for (size_t k = 0; k < Wk.comps.size(); k++) {
        const R1csOpenComp& c = Wk.comps[k];
        for (uint32_t j = 0; j < c.n_wires; j++) Wk.cls[Wk.wires[c.wire0 + j]] = S.h_cls[c.wire0 + j];
        if (!c.n_cross) dims += c.n_wires - std::min<uint64_t>(r1cs_open_rank(r, k), c.n_wires);
    }
    uint64_t count[6] = {0, 0, 0, 0, 0, 0}, listed = 0;
    for (uint32_t i = 0; i < r->n_wires; i++) {
        const uint8_t k = Wk.cls[i];
        count[k]++;
        if (k != K16_OPEN_FIXED && k != K16_OPEN_ABSENT && listed < cap) {
            if (h_wires) h_wires[listed] = i;
            if (h_class) h_class[listed] = k;
            listed++;
        }
    }
    if (h_status) memcpy(h_status, Wk.cls.data(), r->n_wires);
    if (h_comp) memcpy(h_comp, Wk.comp.data(), (size_t)r->n_wires * 4);
    *n_forced     = count[K16_OPEN_FORCED];
    *n_free       = count[K16_OPEN_FREE];
    *n_undecided  = count[K16_OPEN_UNDECIDED];
    *n_skipped    = count[K16_OPEN_SKIPPED];
    *n_absent     = count[K16_OPEN_ABSENT];
    *n_components = Wk.n_components;
    *n_dims       = dims;
    return K16_OK;
}

extern "C" int k16_r1cs_open_system(k16_r1cs* r, const uint8_t* h_fixed, uint64_t* n_forced, uint64_t* n_free, uint64_t* n_undecided,
                                    uint64_t* n_skipped, uint64_t* n_absent, uint64_t* n_components, uint64_t* n_dims, uint32_t* h_wires,
                                    uint8_t* h_class, uint32_t cap, uint8_t* h_status, uint32_t* h_comp)
{
    return k16_guard(r ? r->ctx : nullptr, [&]() -> int {
    if (!r || !n_forced || !n_free || !n_undecided || !n_skipped || !n_absent || !n_components || !n_dims) return K16_ERR_ARG;
    return r1cs_open_system(r, h_fixed, R1CS_OPEN_MAX_WIRES, n_forced, n_free, n_undecided, n_skipped, n_absent, n_components, n_dims, h_wires,
                            h_class, cap, h_status, h_comp);
    });
}

extern "C" int k16_r1cs_open_system_ex(k16_r1cs* r, const uint8_t* h_fixed, uint32_t max_wires, uint64_t* n_forced, uint64_t* n_free,
                                       uint64_t* n_undecided, uint64_t* n_skipped, uint64_t* n_absent, uint64_t* n_components,
                                       uint64_t* n_dims, uint32_t* h_wires, uint8_t* h_class, uint32_t cap, uint8_t* h_status, uint32_t* h_comp)
{
    return k16_guard(r ? r->ctx : nullptr, [&]() -> int {
    if (!r || !n_forced || !n_free || !n_undecided || !n_skipped || !n_absent || !n_components || !n_dims) return K16_ERR_ARG;
    const int rc = r1cs_open_cap(r->ctx, max_wires); // (before the counts are zeroed: a refused cap writes nothing)
    if (rc) return rc;
    return r1cs_open_system(r, h_fixed, max_wires, n_forced, n_free, n_undecided, n_skipped, n_absent, n_components, n_dims, h_wires, h_class,
                            cap, h_status, h_comp);
    });
}

static int r1cs_open_direction(k16_r1cs* r, const uint8_t* h_fixed, uint32_t max_wires, uint32_t wire, uint8_t* cls, uint32_t* comp_wires,
                               uint32_t* comp_rows, uint32_t* comp_cross, uint32_t* rank, uint64_t* n, uint32_t* h_wires, uint8_t* h_vals,
                               uint32_t cap)
{
    *cls = K16_OPEN_FIXED;
    *n   = 0;
    for (uint32_t* p : {comp_wires, comp_rows, comp_cross, rank})
        if (p) *p = 0;
    k16_ctx* ctx = r->ctx;
    if (wire >= r->n_wires) {
        ctx->err = "wire number out of range";
        return K16_ERR_ARG;
    }
    int rc = r1cs_open_begin(ctx, r, h_fixed);
    if (rc) return rc;
    if ((rc = r1cs_open_wide_stage(ctx, r, max_wires))) return rc;
    ScanOpen& S = *r->scans->open;
    uint32_t  nw = 0, nr = 0, nx = 0;
    const uint8_t host = r1cs_open_one(r->scans->pairs, S.index, r->n_wires, r->M, h_fixed, (const uint64_t*)S.h_verdict.p, wire, &S.work, &nw, &nr, &nx,
                                       max_wires);
    if (comp_wires) *comp_wires = nw;
    if (comp_rows) *comp_rows = nr;
    if (comp_cross) *comp_cross = nx;
    *cls = host;
    if (host != R1CS_OPEN_ELIMINATED) return K16_OK;
    const R1csOpenWork& Wk  = S.work;
    const uint32_t      col = (uint32_t)(std::lower_bound(Wk.wires.begin(), Wk.wires.end(), wire) - Wk.wires.begin());
    *cls = K16_OPEN_FIXED;
    if ((rc = r1cs_scan_drained(ctx, r1cs_open_run(ctx, r, true, col)))) return rc;
    *cls = S.h_cls[col];
    if (rank) *rank = (uint32_t)r1cs_open_rank(r, 0);
    if (*cls != K16_OPEN_FREE) return K16_OK;
    const bool     is_wide = nw > R1CS_OPEN_MAX_WIRES;
    const Fr*      emit    = is_wide ? r->scans->open_wide->h_emit.p : S.h_emit.p;
    const uint32_t width   = is_wide ? R1CS_OPEN_MAX_WIRES_EX : R1CS_OPEN_MAX_WIRES;
    uint64_t found = 0;
    for (uint32_t j = 0; j < nw && j < width; j++) {
        const Fr& v = emit[j];
        if (!(v.v[0] | v.v[1] | v.v[2] | v.v[3] | v.v[4] | v.v[5] | v.v[6] | v.v[7])) continue;
        if (found < cap) {
            if (h_wires) h_wires[found] = Wk.wires[j];
            if (h_vals) memcpy(h_vals + 32 * found, v.v, 32);
        }
        found++;
    }
    *n = found;
    return K16_OK;
}

extern "C" int k16_r1cs_open_direction(k16_r1cs* r, const uint8_t* h_fixed, uint32_t wire, uint8_t* cls, uint32_t* comp_wires,
                                       uint32_t* comp_rows, uint32_t* comp_cross, uint32_t* rank, uint64_t* n, uint32_t* h_wires,
                                       uint8_t* h_vals, uint32_t cap)
{
    return k16_guard(r ? r->ctx : nullptr, [&]() -> int {
    if (!r || !cls || !n) return K16_ERR_ARG;
    return r1cs_open_direction(r, h_fixed, R1CS_OPEN_MAX_WIRES, wire, cls, comp_wires, comp_rows, comp_cross, rank, n, h_wires, h_vals, cap);
    });
}

extern "C" int k16_r1cs_open_direction_ex(k16_r1cs* r, const uint8_t* h_fixed, uint32_t max_wires, uint32_t wire, uint8_t* cls,
                                          uint32_t* comp_wires, uint32_t* comp_rows, uint32_t* comp_cross, uint32_t* rank, uint64_t* n,
                                          uint32_t* h_wires, uint8_t* h_vals, uint32_t cap)
{
    return k16_guard(r ? r->ctx : nullptr, [&]() -> int {
    if (!r || !cls || !n) return K16_ERR_ARG;
    const int rc = r1cs_open_cap(r->ctx, max_wires); // (before *cls and *n are written: a refused cap writes nothing)
    if (rc) return rc;
    return r1cs_open_direction(r, h_fixed, max_wires, wire, cls, comp_wires, comp_rows, comp_cross, rank, n, h_wires, h_vals, cap);
    });
}

// ---- the list itself
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
    const R1csPairs& P = r->scans->pairs;
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
    *n_pairs = r->scans->pairs.n_pairs();
    return K16_OK;
    });
}
