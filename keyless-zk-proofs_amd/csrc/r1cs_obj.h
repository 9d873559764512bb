// r1cs_obj.h -- internal: the R1CS object (include/k16.h k16_r1cs) as r1cs_check.hip and r1cs_scan.hip share it, and the two
// owners every one of its buffers lives in.  The check owns the circuit on the device, the buffers of a check and the record a
// prove call reads (k16_r1cs_create_mem, k16_r1cs_attach).  The diagnostics read d_coef, d_rows and d_mask of a completed check;
// what they add hangs off `scans`, a type only r1cs_scan.hip knows: made by the first call that needs it, kept until the object goes.
#pragma once
#include <memory>
#include <utility>
#include "ctx.h"
#include "r1cs_file.h"

namespace k16 {

// hipMalloc memory, freed with its owner on the device that is current then.  Move-only; alloc: on an empty owner.
template <class T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)) {}
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc((void**)&p, bytes); }
    operator T*() const { return p; }
};
// hipHostMalloc memory; dev: its device alias where the flags ask for mapped memory
template <class T>
struct PinnedBuf {
    T *p = nullptr, *dev = nullptr;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), dev(std::exchange(o.dev, nullptr)) {}
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t bytes, unsigned flags = hipHostMallocDefault)
    {
        const hipError_t e = hipHostMalloc((void**)&p, bytes, flags);
        return e == hipSuccess && (flags & hipHostMallocMapped) ? hipHostGetDevicePointer((void**)&dev, p, 0) : e;
    }
    operator T*() const { return p; }
    T* operator->() const { return p; }
};

// why a witness is refused (k_r1cs_wtns; the witness completion's k_r1cs_solve_mask): bits of the flag word behind the verdicts
enum : unsigned long long { WTNS_NOT_BELOW_R = 1, WTNS_WIRE0_NOT_ONE = 2 };

// What a prove call keeps of its check (pinned, device-mapped; read by the host after the check is joined).
struct CheckRecord {
    unsigned long long flags;                       // WTNS_* of k_r1cs_wtns
    unsigned long long count;                       // exact number of broken constraints
    uint32_t           lowest[K16_R1CS_REPORT_MAX]; // the lowest min(count, K16_R1CS_REPORT_MAX) of them, ascending
};

struct R1csScans; // r1cs_scan.hip: the host list, the device list, the second-value, the closure and the completion buffers
void r1cs_scans_delete(R1csScans* s);

} // namespace k16

struct k16_r1cs {
    k16_ctx*      ctx = nullptr;
    k16::R1csFile file; // the host copy: k16_r1cs_match_zkey compares it with a key
    uint32_t      n_wires = 0, n_public = 0, M = 0, n_words = 0;
    // the circuit on the device (see k_r1cs_rows)
    k16::DevBuf<k16::SpmvSlice> d_slices;
    k16::DevBuf<k16::SpmvLong>  d_longs;
    k16::DevBuf<uint32_t>       d_rowof, d_wire;
    k16::DevBuf<k16::Fr>        d_coef; // coefficient * 2^522 mod r, as the prover stores its own
    uint32_t                    n_slices = 0, n_long = 0;
    uint64_t                    n_entries = 0; // of the plan d_coef was laid out by (r1cs_scan.hip names coefficients by position in it)
    // per check
    k16::DevBuf<k16::Fr>                  d_wtns; // an uploaded witness (k16_r1cs_check_mem / _file)
    k16::DevBuf<uint16_t>                 d_n16;
    k16::DevBuf<k16::Fr>                  d_rows; // [3 M]
    k16::DevBuf<unsigned long long>       d_mask; // [n_words] verdicts | [1] witness flags
    k16::PinnedBuf<unsigned long long>    h_mask; // pinned copy
    bool                                  have_values = false; // d_rows holds the sums of a completed check (k16_r1cs_last_values)
    // attached to a prover (k16_r1cs_attach): made by the first attach, kept until the object goes
    k16::PinnedBuf<k16::CheckRecord> rec;                 // pinned, device-mapped
    hipStream_t                      forked_on = nullptr; // the prover's stream a check is (or may be) in flight on; null: none
    // the diagnostics of r1cs_scan.hip
    std::unique_ptr<k16::R1csScans, void (*)(k16::R1csScans*)> scans{nullptr, k16::r1cs_scans_delete};

    // A check a prover forked may still write the record: it is waited for before any member is released.
    ~k16_r1cs()
    {
        if (ctx) (void)hipSetDevice(ctx->device);
        if (forked_on) (void)hipStreamSynchronize(forked_on);
    }
};
