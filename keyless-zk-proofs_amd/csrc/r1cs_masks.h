// r1cs_masks.h -- host side of the diagnostics of r1cs_scan.hip: from the bit masks a scan leaves to what its call returns.
// Pure C++ (no HIP): compiled into libk16.so and, on its own, into tests/cpp/r1cs_masks_check.cpp.
// A mask has ceil(n_wires / 64) words, bit i % 64 of word i / 64 for wire i; bits at or above n_wires count for nothing.
// `present` is R1csPairs::present: the wire has a column.  Every call gives exact counts, the wires it names in ascending order
// cut at `cap`, and one status byte per wire (include/k16.h K16_WIRE_*, K16_DET_*).  A list or status pointer may be null: the
// counts are always made, a list that has nowhere to go is not walked.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include "../../include/k16.h"

namespace k16 {

// Word w of a mask over n_wires wires: in_word wires live in it (0: the mask has ended), `valid` holds their bits.
struct R1csMaskWord {
    size_t             w;
    uint32_t           in_word;
    unsigned long long valid;
    R1csMaskWord(uint32_t n_wires, size_t w_)
        : w(w_), in_word((uint32_t)std::min<uint64_t>(64, n_wires - std::min<uint64_t>(n_wires, 64 * (uint64_t)w_))),
          valid(in_word == 64 ? ~0ull : (1ull << in_word) - 1)
    {
    }
    R1csMaskWord next(uint32_t n_wires) const { return R1csMaskWord(n_wires, w + 1); }
};
// a wire that no constraint binds: has it a column?  here: the word of `present`
inline uint8_t r1cs_free_class(unsigned long long here, uint32_t b) { return (here >> b) & 1 ? K16_WIRE_UNBOUND : K16_WIRE_ABSENT; }
// The set bits of m, word w of a mask, ascending, while the list holds fewer than cap: their wires to wires[listed ..], their classes
// as free wires to cls[listed ..]; either may be null.  Returns the new length.
inline uint64_t r1cs_mask_list(size_t w, unsigned long long m, uint64_t listed, uint64_t cap, uint32_t* wires, uint8_t* cls = nullptr,
                               unsigned long long here = 0)
{
    for (; m && listed < cap; m &= m - 1, listed++) {
        const uint32_t b = (uint32_t)__builtin_ctzll(m);
        if (wires) wires[listed] = (uint32_t)(64 * w + b);
        if (cls) cls[listed] = r1cs_free_class(here, b);
    }
    return listed;
}

// The unbound-wire scan.  bound: bit i = some constraint binds wire i.  Wire 0, the constant, is bound by definition.
inline void r1cs_masks_unbound(uint32_t n_wires, const uint64_t* present, const unsigned long long* bound, uint64_t* n_absent,
                               uint64_t* n_unbound, uint32_t* h_wires, uint8_t* h_class, uint32_t cap, uint8_t* h_status)
{
    uint64_t absent = 0, unbound = 0, listed = 0;
    for (R1csMaskWord k(n_wires, 0); k.in_word; k = k.next(n_wires)) {
        const unsigned long long free_ = ~bound[k.w] & k.valid & ~(unsigned long long)(k.w == 0), here = present[k.w];
        absent += (uint64_t)__builtin_popcountll(free_ & ~here);
        unbound += (uint64_t)__builtin_popcountll(free_ & here);
        for (uint32_t b = 0; h_status && b < k.in_word; b++) h_status[64 * k.w + b] = (free_ >> b) & 1 ? r1cs_free_class(here, b) : K16_WIRE_BOUND;
        if (h_wires || h_class) listed = r1cs_mask_list(k.w, free_, listed, cap, h_wires, h_class, here);
    }
    *n_absent = absent, *n_unbound = unbound;
}

// The second-value scan.  pinned / rooted: bit i = wire i has a PIN / a ROOT incidence (a clash among ROOTs is a PIN): it is
// two-valued when rooted and not pinned, and bound -- as the unbound-wire scan finds it -- when either.  list (null: nothing is
// listed) takes the lowest min(count, cap) two-valued wires; their number is returned.
inline uint32_t r1cs_masks_second(uint32_t n_wires, const uint64_t* present, const unsigned long long* pinned, const unsigned long long* rooted,
                                  uint64_t* n_two_valued, uint32_t* list, uint32_t cap, uint8_t* h_status)
{
    uint64_t count = 0, listed = 0;
    for (R1csMaskWord k(n_wires, 0); k.in_word; k = k.next(n_wires)) {
        const unsigned long long valid = k.valid & ~(unsigned long long)(k.w == 0); // wire 0 is the constant
        const unsigned long long free_ = ~(pinned[k.w] | rooted[k.w]) & valid, here = present[k.w], two = rooted[k.w] & ~pinned[k.w] & valid;
        count += (uint64_t)__builtin_popcountll(two);
        for (uint32_t b = 0; h_status && b < k.in_word; b++)
            h_status[64 * k.w + b] = (two >> b) & 1 ? K16_WIRE_TWO_VALUED : (free_ >> b) & 1 ? r1cs_free_class(here, b) : K16_WIRE_BOUND;
        if (list) listed = r1cs_mask_list(k.w, two, listed, cap, list);
    }
    *n_two_valued = count;
    return (uint32_t)listed;
}

// The seed of the determinism closure: wire 0, and either the n_seed wires of h_seed (any order, duplicates allowed) or, with
// h_seed null, what the file's header calls inputs, in the iden3 wire order 1 | public outputs | public inputs | private inputs.
// Returns null, or why the seed is refused (nothing is written then).
inline const char* r1cs_seed_mask(uint32_t n_wires, uint32_t n_pub_out, uint32_t n_pub_in, uint32_t n_prv_in, const uint32_t* h_seed,
                                  uint32_t n_seed, unsigned long long* seed)
{
    const uint64_t in0 = (uint64_t)n_pub_out + 1, in1 = in0 + n_pub_in + n_prv_in;
    if (!h_seed && in1 > n_wires) return "the header's input wires reach beyond nWires";
    for (uint32_t k = 0; h_seed && k < n_seed; k++)
        if (h_seed[k] >= n_wires) return "seed wire number out of range";
    memset(seed, 0, (((size_t)n_wires + 63) / 64) * 8);
    seed[0] = 1ull; // wire 0
    for (uint32_t k = 0; h_seed && k < n_seed; k++) seed[h_seed[k] >> 6] |= 1ull << (h_seed[k] & 63u);
    for (uint64_t i = in0; !h_seed && i < in1; i++) seed[i >> 6] |= 1ull << (i & 63u);
    return nullptr;
}

// The determinism closure.  seed / known: bit i = wire i is in the seed / in the closure, which holds the seed.  h_wires takes the
// lowest min(n_open, cap) open wires; h_round, the rounds as the device left them, gets round 0 for the seed wires.
inline void r1cs_masks_closure(uint32_t n_wires, const uint64_t* present, const unsigned long long* seed, const unsigned long long* known,
                               uint64_t* n_derived, uint64_t* n_absent, uint64_t* n_open, uint32_t* h_wires, uint32_t cap, uint8_t* h_status,
                               uint32_t* h_round)
{
    uint64_t derived = 0, absent = 0, open = 0, listed = 0;
    for (R1csMaskWord k(n_wires, 0); k.in_word; k = k.next(n_wires)) {
        const unsigned long long here = present[k.w], in = seed[k.w], out = ~known[k.w] & k.valid, got = known[k.w] & ~in & k.valid;
        derived += (uint64_t)__builtin_popcountll(got);
        absent += (uint64_t)__builtin_popcountll(out & ~here);
        open += (uint64_t)__builtin_popcountll(out & here);
        for (uint32_t b = 0; h_status && b < k.in_word; b++)
            h_status[64 * k.w + b] = (in >> b) & 1 ? K16_DET_SEED : (got >> b) & 1 ? K16_DET_DERIVED : (here >> b) & 1 ? K16_DET_OPEN : K16_DET_ABSENT;
        for (unsigned long long m = h_round ? in & k.valid : 0; m; m &= m - 1) h_round[64 * k.w + (uint32_t)__builtin_ctzll(m)] = 0;
        if (h_wires) listed = r1cs_mask_list(k.w, out & here, listed, cap, h_wires);
    }
    *n_derived = derived, *n_absent = absent, *n_open = open;
}

} // namespace k16
