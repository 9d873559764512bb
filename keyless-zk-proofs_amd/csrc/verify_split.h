// verify_split.h -- what the prover (prover.hip) needs of a verification key (verify.hip) for k16_prover_prove_*_verified:
// the split check of ONE proof on the key's own stream, through the key's pinned, device-mapped buffer.
//   begin   takes the key's split buffers (one verified prove at a time per key) and stores the public inputs
//   early   A and B are final: point checks, vk_x and the Miller loops of (A, B), (vk_x, -gamma) -- launched, not waited for
//   late    C is final: its point check, the Miller loop of (C, -delta), the product, the final exponentiation; waits
//   end     waits for whatever is still in flight on the key's stream and gives the buffers back
// early / late return K16_OK, a negative error, or K16_SPLIT_UNDECIDED: a zero point, vk_x at infinity or a key without the
// programs -- k16_verify_batch settles the proof after the prove call (same flag).
#pragma once
#include <stdint.h>
#include "bn254_curve.h"

struct k16_ctx;
struct k16_vk;

namespace k16 {
constexpr int K16_SPLIT_UNDECIDED = 1;
k16_ctx*      vk_split_ctx(const k16_vk* vk);
uint32_t      vk_split_n_ic(const k16_vk* vk);
int           vk_split_begin(const k16_vk* vk, const uint8_t* inputs /* (n_ic - 1) x 32 B */);
int           vk_split_early(const k16_vk* vk, const G1Aff& A, const G2Aff& B);
int           vk_split_late(const k16_vk* vk, const G1Aff& C, uint8_t* out_ok);
void          vk_split_end(const k16_vk* vk);
} // namespace k16
