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
// The diagnostics that read the sums and the verdicts a completed check leaves behind live in r1cs_scan.hip.
#include <stdio.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>
#include "r1cs_obj.h"
#include "spmv_dev.h"

using namespace k16;

static_assert(R1CS_ERR_ARG == K16_ERR_ARG && R1CS_ERR_FORMAT == K16_ERR_FORMAT && R1CS_ERR_CURVE == K16_ERR_CURVE && R1CS_OK == K16_OK,
              "r1cs_file.h returns the library's status codes");

namespace {

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
        fail = fr9_nonzero(frsub9(frmul9(ld_r9(&rows[i]), ld_r9(&rows[(size_t)M + i])), ld_r9(&rows[2 * (size_t)M + i])));
    }
    const unsigned long long votes = __ballot(fail);
    if ((threadIdx.x & 63u) == 0 && (i >> 6) < n_words) mask[i >> 6] = votes;
}

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

void k16_r1cs_view(const k16_r1cs* r, k16_ctx** ctx, const R1csFile** file)
{
    *ctx  = r->ctx;
    *file = &r->file;
}

// the circuit and the buffers of a check on the device; the uploads are queued on the context's stream and waited for
static int r1cs_upload(k16_ctx* ctx, k16_r1cs* r, const SpmvPlan& pl, const std::vector<uint32_t>& wire, const std::vector<R1csFr>& vals)
{
    K16_HIP(ctx, hipSetDevice(ctx->device));
    K16_HIP(ctx, r->d_slices.alloc(pl.slices.size() * sizeof(SpmvSlice)));
    K16_HIP(ctx, r->d_longs.alloc(pl.longs.size() * sizeof(SpmvLong)));
    K16_HIP(ctx, r->d_rowof.alloc(pl.row_of.size() * 4));
    K16_HIP(ctx, r->d_wire.alloc(wire.size() * 4));
    K16_HIP(ctx, r->d_coef.alloc(vals.size() * 32));
    K16_HIP(ctx, r->d_wtns.alloc((size_t)r->n_wires * 32));
    K16_HIP(ctx, r->d_n16.alloc((size_t)r->n_wires * 2 + 64));
    K16_HIP(ctx, r->d_rows.alloc(std::max<size_t>(3 * (size_t)r->M, 1) * 32));
    K16_HIP(ctx, r->d_mask.alloc(((size_t)r->n_words + 1) * 8));
    K16_HIP(ctx, r->h_mask.alloc(((size_t)r->n_words + 1) * 8));
    hipStream_t st = ctx->stream;
    K16_HIP(ctx, hipMemcpyAsync(r->d_slices, pl.slices.data(), pl.slices.size() * sizeof(SpmvSlice), hipMemcpyHostToDevice, st));
    K16_HIP(ctx, hipMemcpyAsync(r->d_longs, pl.longs.data(), pl.longs.size() * sizeof(SpmvLong), hipMemcpyHostToDevice, st));
    K16_HIP(ctx, hipMemcpyAsync(r->d_rowof, pl.row_of.data(), pl.row_of.size() * 4, hipMemcpyHostToDevice, st));
    K16_HIP(ctx, hipMemcpyAsync(r->d_wire, wire.data(), wire.size() * 4, hipMemcpyHostToDevice, st));
    K16_HIP(ctx, hipMemcpyAsync(r->d_coef, vals.data(), vals.size() * 32, hipMemcpyHostToDevice, st));
    K16_HIP(ctx, hipStreamSynchronize(st));
    return K16_OK;
}

extern "C" int k16_r1cs_create_mem(k16_ctx* ctx, const void* r1cs, size_t size, k16_r1cs** out)
{
    return k16_guard(ctx, [&]() -> int {
    if (!ctx || !r1cs || !out) return K16_ERR_ARG;
    *out = nullptr;
    std::unique_ptr<k16_r1cs> r(new k16_r1cs()); // owns every buffer: whatever fails below, all of it goes with the object
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
    if ((rc = r1cs_upload(ctx, r.get(), plan.plan, wire, vals))) {
        (void)hipStreamSynchronize(ctx->stream); // uploads from the local vectors may be queued
        return rc;
    }
    *out = r.release();
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
        delete r;
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

int k16_r1cs_launch(k16_r1cs* r, hipStream_t st, const Fr* d_wtns) { return r1cs_launch(r->ctx, r, d_wtns, nullptr, st); }

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
    if (!r->rec) K16_HIP(ctx, r->rec.alloc(sizeof(CheckRecord), hipHostMallocMapped | hipHostMallocCoherent));
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
        hipLaunchKernelGGL(k_r1cs_summary, dim3(1), dim3(256), 0, st, r->d_mask, r->n_words, r->rec.dev);
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
    const CheckRecord* rec = r->rec;
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
        static const char* const where[] = {"", "header", "matrix A", "matrix B", "public rows"};
        char                     buf[256];
        snprintf(buf, sizeof buf, "r1cs / zkey mismatch: %s, constraint %u, wire %u (%s)", where[mm.kind], mm.constraint, mm.wire, why);
        ctx->err = buf;
    }
    return K16_OK;
    });
}
