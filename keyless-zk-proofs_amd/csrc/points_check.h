// points_check.h -- the batched point checks of points_check.hip, for the other units of the library (verify.hip:
// k16_verify_batch_checked; prover.hip: k16_zkey_check).  The C ABI is include/k16.h (k16_points_check and the two above).
#pragma once
#include "ctx.h"
#include "bn254_points.h"

namespace k16 {

// twist_b, twqx, twqy in Montgomery form (computed once per process; verify.hip, which holds the pairing constants)
const G2Consts& g2_consts_host();

// Streams points from host memory through two bounded device buffers (PTS_CHUNK_BYTES each): the copy of chunk k + 1 (its
// own stream) overlaps the check of chunk k (the context's stream).  A failing point either gets its status written to
// h_status (may be NULL), or is counted and folded into the smallest key  key_base + (index << 2 | status)  -- the first
// failure in (section, index) order when key_base = section << 56.
constexpr uint64_t PTS_CHUNK_BYTES = 32ull << 20;
struct PointsStream {
    k16_ctx*    ctx = nullptr;
    hipStream_t copy = nullptr;
    hipEvent_t  copied[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
    uint8_t*    d_pts[2]  = {nullptr, nullptr};
    uint8_t *   h_st[2] = {nullptr, nullptr}, *d_st[2] = {nullptr, nullptr}; // pinned, device-mapped status of a chunk
    uint64_t*   d_sum = nullptr;                                               // [0] smallest key, [1] failures
    size_t      cap = 0;                                                       // bytes per buffer
    uint64_t    k   = 0;                                                       // chunks issued
    // the chunk issued into buffer b and not yet drained: where its statuses go
    uint8_t*    pend_out[2] = {nullptr, nullptr};
    uint64_t    pend_n[2]   = {0, 0};
    bool        pend[2]     = {false, false};

    int  begin(k16_ctx* c, size_t max_bytes);
    int  feed(int group, const uint8_t* h_pts, uint64_t n, uint8_t* h_status, uint64_t key_base);
    int  finish(uint64_t* first_key, uint64_t* n_bad); // waits for everything; first_key = ~0 when nothing failed
    ~PointsStream();

  private:
    int drain(int b);
};

// reason[i] = the status of proof i's first failing point (A, then B, then C), 0 if all pass: one launch for the batch,
// a lane pair per proof.  d_proofs: n x 256 B (A | B | C), device-readable.
int launch_proofs_check(hipStream_t st, const uint8_t* d_proofs, uint64_t n, uint8_t* d_reason);

} // namespace k16
