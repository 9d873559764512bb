// setup.hip -- set-up from a trapdoor (include/k16.h, k16_r1cs_setup* and k16_generator_mul): a Groth16 proving key for any
// .r1cs, made on the GPU from known tau, alpha, beta, gamma, delta.  DEVELOPMENT AND TEST MATERIAL: whoever holds the trapdoor
// can forge proofs.  Formulas and layout: setup_plan.h, DESIGN.md section 11.
//   k_setup_lagrange  L_j(t) = (t^N - 1)/N * w^j / (t - w^j) for j < N at t = tau and t = tau / g, in the prover's Fr code (packed
//                     R' values).  A lane owns LAG_CHUNK consecutive j: w^j0 by square-and-multiply, the denominators' prefix
//                     products parked in the output, ONE inversion per lane (Montgomery's trick), the quotients on the way back.
//   k_setup_columns   spmv_walk over the transposed matrices (setup_plan.h): the 3 nWires sums a_i | b_i | c_i at tau, with
//                     L(tau) in the witness's place and no n16.
//   k_setup_scalars   one pointwise pass: a_i, b_i, (beta a_i + alpha b_i + c_i) / gamma or / delta, Z(tau) L_i(tau / g) / (-2 delta),
//                     all in standard form -- the scalars of sections 3, 5 .. 9.
//   k_genmul          scalar * generator through a window table of the generator: ceil(256 / w) COMPLETE mixed additions per point
//                     in the MSM kernels' representation (Fq9 for G1, Fq2n for G2), any 256-bit scalar, one inversion per
//                     GENMUL_CHUNK points of a lane.
// Why the complete addition: the accumulator after the windows below k is (s mod 2^(w k)) G and the table entry is
// d 2^(w k) G.  For s >= r the two scalars can be congruent mod r (the addition doubles) or opposite (it cancels), e.g.
// s = r + 2 d0 or s = r; padd_mixed9 / padd_mixed test P = 0 and take pdbl_aff, and P = 0 with R != 0 gives ZZ3 = 0, the
// point at infinity, which the next addition takes as its first branch.  The bucket accumulation's shortcut forms do not.
#include <stdio.h>
#include <string.h>
#include <unistd.h>
#include <string>
#include <vector>
#include "ctx.h"
#include "frinv_dev.h"
#include "setup_plan.h"
#include "spmv_dev.h"

using namespace k16;

namespace {

constexpr unsigned GENMUL_W[2]     = {10, 9}; // G1: 26 windows, 1.7 MB; G2: 29 windows, 1.9 MB -- both stay in a 4 MB L2
constexpr unsigned GENMUL_CHUNK[2] = {8, 2};  // points per lane and inversion
constexpr uint64_t GENMUL_BATCH[2] = {1ull << 21, 1ull << 20}; // points per launch (bounds the scratch area: 302 MB)
constexpr unsigned LAG_CHUNK       = 16;
constexpr unsigned genmul_windows(int group) { return (256 + GENMUL_W[group] - 1) / GENMUL_W[group]; }

struct LagArgs {
    Fr t, c, omega, omega_inv; // packed R': the point, (t^N - 1) / N, the domain's generator and its inverse
};
// out: [2][N] packed R'; blockIdx.y = 0: at a0.t (tau), 1: at a1.t (tau / g).  t^(2N) != 1, so no denominator vanishes.
__global__ void __launch_bounds__(64) k_setup_lagrange(LagArgs a0, LagArgs a1, uint32_t N, Fr* __restrict__ out)
{
    const LagArgs& a  = blockIdx.y ? a1 : a0;
    Fr*            o  = out + (size_t)blockIdx.y * N;
    const uint64_t j0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * LAG_CHUNK;
    if (j0 >= N) return;
    const uint64_t j1 = j0 + LAG_CHUNK < N ? j0 + LAG_CHUNK : N;
    const Fr9      t = ld_r9(&a.t), om = ld_r9(&a.omega), omi = ld_r9(&a.omega_inv), c = ld_r9(&a.c);
    Fr9            w = fr9_one();
#pragma clang loop unroll(disable)
    for (int bit = 31; bit >= 0; bit--) {
        w = frmul9(w, w);
        if ((j0 >> bit) & 1u) w = frmul9(w, om);
    }
    Fr9 prod = fr9_one();
#pragma clang loop unroll(disable)
    for (uint64_t j = j0; j < j1; j++) {
        st_r9(&o[j], prod);
        prod = frmul9(prod, frsub9(t, w));
        w    = frmul9(w, om);
    }
    Fr9 inv = frinv9(prod);
#pragma clang loop unroll(disable)
    for (uint64_t j = j1; j-- > j0;) {
        w              = frmul9(w, omi);
        const Fr9 dinv = frmul9(inv, ld_r9(&o[j]));
        inv            = frmul9(inv, frsub9(t, w));
        st_r9(&o[j], frmul9(frmul9(c, w), dinv));
    }
}

__global__ void __launch_bounds__(256) k_setup_columns(const SpmvSlice* __restrict__ slices, uint32_t n_slices,
                                                       const uint32_t* __restrict__ row_of, const SpmvLong* __restrict__ longs,
                                                       uint32_t n_long, const uint32_t* __restrict__ cons,
                                                       const Fr* __restrict__ coef9, const Fr* __restrict__ lag, Fr* __restrict__ cols)
{
    spmv_walk(slices, n_slices, row_of, longs, n_long, cons, coef9, lag, nullptr,
              [&](uint32_t row, const Fr9& acc) { st_r9(&cols[row], acc); });
}

struct MixArgs {
    Fr alpha, beta, gamma_inv, delta_inv, hk; // packed R'; hk = Z(tau) / (-2 delta)
};
// cols: a | b | c, nw packed R' values each; lagc: L(tau / g).  Outputs in standard form, 32 B each.
__global__ void __launch_bounds__(256) k_setup_scalars(const Fr* __restrict__ cols, uint32_t nw, uint32_t n_public,
                                                       const Fr* __restrict__ lagc, uint32_t N, MixArgs m, Fr* __restrict__ s_a,
                                                       Fr* __restrict__ s_b, Fr* __restrict__ s_ic, Fr* __restrict__ s_c,
                                                       Fr* __restrict__ s_h)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nw) {
        const Fr9 a = ld_r9(&cols[i]), b = ld_r9(&cols[(size_t)nw + i]), c = ld_r9(&cols[2 * (size_t)nw + i]);
        st_fr(&s_a[i], fr9_to_standard(a));
        st_fr(&s_b[i], fr9_to_standard(b));
        const Fr9 mix = fradd9(fradd9(frmul9(ld_r9(&m.beta), a), frmul9(ld_r9(&m.alpha), b)), c);
        if (i <= n_public)
            st_fr(&s_ic[i], fr9_to_standard(frmul9(mix, ld_r9(&m.gamma_inv))));
        else
            st_fr(&s_c[i - n_public - 1], fr9_to_standard(frmul9(mix, ld_r9(&m.delta_inv))));
    }
    if (i < N) st_fr(&s_h[i], fr9_to_standard(frmul9(ld_r9(&m.hk), ld_r9(&lagc[i]))));
}

// ---------------------------------------------------------------- scalar * generator
// The two groups through one kernel body: field F of the coordinates, accumulator and table entry.
struct GenG1 {
    typedef Fq9   F;
    typedef Xyzz9 Acc;
    typedef G1Aff Out;
    static constexpr int GROUP = 0, ENTRY_WORDS = 16;
    static __device__ __forceinline__ F    one() { return fq9_one(); }
    static __device__ __forceinline__ F    zero() { return fq9_zero(); }
    static __device__ __forceinline__ F    mul(const F& a, const F& b) { return fmul9(a, b); }
    static __device__ __forceinline__ F    inv(const F& a) { return finv9(a); }
    static __device__ __forceinline__ Acc  acc_zero() { return Xyzz9::zero(); }
    static __device__ __forceinline__ void madd(Acc& acc, const uint32_t* __restrict__ e)
    {
        uint32_t w[16];
        const uint4* s = reinterpret_cast<const uint4*>(e);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint4 v = s[k];
            w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
        acc = padd_mixed9(acc, Aff9{fq9_unpack(w), fq9_unpack(w + 8)});
    }
    static __device__ __forceinline__ Out out(const F& x, const F& y) { return G1Aff{fq9_to_fq(x), fq9_to_fq(y)}; }
    static __device__ __forceinline__ void entry(uint32_t* __restrict__ e, const G1Aff& p)
    {
        fq9_pack(e, fq9_from_fq(p.x));
        fq9_pack(e + 8, fq9_from_fq(p.y));
    }
};
struct GenG2 {
    typedef Fq2n       F;
    typedef Xyzz<Fq2n> Acc;
    typedef G2Aff      Out;
    static constexpr int GROUP = 1, ENTRY_WORDS = 32;
    static __device__ __forceinline__ F    one() { return Fq2n::one(); }
    static __device__ __forceinline__ F    zero() { return Fq2n::zero(); }
    static __device__ __forceinline__ F    mul(const F& a, const F& b) { return fmul(a, b); }
    static __device__ __forceinline__ F    inv(const F& x)
    {
        const Fq9 t = finv9(fred9(fadd9(fsqr9(x.a), fsqr9(x.b)))); // f2field.cpp:178-190: (a - bu) / (a^2 + b^2)
        return Fq2n{fmul9(x.a, t), fmul9(fsub9<4>(fq9_zero(), x.b), t)};
    }
    static __device__ __forceinline__ Acc  acc_zero() { return Xyzz<Fq2n>::zero(); }
    static __device__ __forceinline__ void madd(Acc& acc, const uint32_t* __restrict__ e)
    {
        uint32_t w[32];
        const uint4* s = reinterpret_cast<const uint4*>(e);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint4 v = s[k];
            w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
        acc = padd_mixed(acc, Aff<Fq2n>{Fq2n{fq9_unpack(w), fq9_unpack(w + 8)}, Fq2n{fq9_unpack(w + 16), fq9_unpack(w + 24)}});
    }
    static __device__ __forceinline__ Out out(const F& x, const F& y) { return G2Aff{fq2n_to_canonical(x), fq2n_to_canonical(y)}; }
    static __device__ __forceinline__ void entry(uint32_t* __restrict__ e, const G2Aff& p)
    {
        fq9_pack(e, fq9_from_fq(p.x.a));
        fq9_pack(e + 8, fq9_from_fq(p.x.b));
        fq9_pack(e + 16, fq9_from_fq(p.y.a));
        fq9_pack(e + 24, fq9_from_fq(p.y.b));
    }
};

// scalars of the table's entries: entry k * 2^w + d is d * 2^(w k), cut to 256 bits; a digit the top window cannot hold is 0
__global__ void __launch_bounds__(256) k_genmul_table_scalars(unsigned w, unsigned n_windows, uint32_t* __restrict__ scalars)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (n_windows << w)) return;
    const unsigned k = i >> w, bit = k * w;
    uint64_t       d = i & ((1u << w) - 1);
    if (bit + w > 256) d = (d >> (256 - bit)) ? 0 : d;
    const uint64_t v = d << (bit & 31); // w <= 16: fits
    for (unsigned j = 0; j < 8; j++) {
        uint32_t x = 0;
        if (j == (bit >> 5)) x = (uint32_t)v;
        if (j == (bit >> 5) + 1) x = (uint32_t)(v >> 32);
        scalars[8 * (size_t)i + j] = x;
    }
}
// canonical affine Montgomery -> the table's packed R' coordinates ((0,0) stays all-zero)
template <class G>
__global__ void __launch_bounds__(256) k_genmul_table_pack(const typename G::Out* __restrict__ pts, uint32_t n, uint32_t* __restrict__ table)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) G::entry(table + (size_t)i * G::ENTRY_WORDS, pts[i]);
}

// out[i] = scalars[i] * G for i < n.  Lane l of the launch's n_lanes owns the points l + q * n_lanes, q < CHUNK; scratch holds
// per (q, lane) x * zzz | y * zz | zz * zzz | the product of the zz * zzz before it: with t = 1 / (zz zzz) the affine point is
// (x zzz t, y zz t).  A point at infinity enters the product as 1 and leaves as (0, 0).
template <class G, unsigned W, unsigned CHUNK>
__global__ void __launch_bounds__(64) k_genmul(const uint32_t* __restrict__ table, const uint32_t* __restrict__ scalars, uint64_t n,
                                               uint64_t n_lanes, typename G::F* __restrict__ scratch,
                                               typename G::Out* __restrict__ out)
{
    typedef typename G::F F;
    const uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= n_lanes || lane >= n) return;
    constexpr unsigned NW = (256 + W - 1) / W;
    F                  prod = G::one();
#pragma clang loop unroll(disable)
    for (unsigned q = 0; q < CHUNK; q++) {
        const uint64_t i = lane + q * n_lanes;
        if (i >= n) break;
        const uint32_t*  s   = scalars + 8 * i;
        typename G::Acc acc = G::acc_zero();
#pragma clang loop unroll(disable)
        for (unsigned k = 0; k < NW; k++) {
            const unsigned bit = k * W, wd = bit >> 5;
            const uint64_t two = (uint64_t)s[wd] | (wd < 7 ? (uint64_t)s[wd + 1] << 32 : 0ull);
            const uint32_t d   = (uint32_t)(two >> (bit & 31)) & ((1u << W) - 1);
            if (d) G::madd(acc, table + (((size_t)k << W) + d) * G::ENTRY_WORDS);
        }
        const bool inf = acc.is_zero();
        F*         sc  = scratch + (size_t)q * 4 * n_lanes + lane;
        const F    m   = inf ? G::one() : G::mul(acc.zz, acc.zzz);
        sc[0]            = inf ? G::zero() : G::mul(acc.x, acc.zzz);
        sc[n_lanes]      = inf ? G::zero() : G::mul(acc.y, acc.zz);
        sc[2 * n_lanes]  = m;
        sc[3 * n_lanes]  = prod;
        prod             = G::mul(prod, m);
    }
    F inv = G::inv(prod);
#pragma clang loop unroll(disable)
    for (unsigned q = CHUNK; q-- > 0;) {
        const uint64_t i = lane + q * n_lanes;
        if (i >= n) continue;
        const F* sc = scratch + (size_t)q * 4 * n_lanes + lane;
        const F  t  = G::mul(inv, sc[3 * n_lanes]);
        inv         = G::mul(inv, sc[2 * n_lanes]);
        out[i]      = G::out(G::mul(sc[0], t), G::mul(sc[n_lanes], t));
    }
}

template <class G>
int genmul_table(k16_ctx* ctx)
{
    if (ctx->gen_table[G::GROUP]) return K16_OK;
    constexpr unsigned w = GENMUL_W[G::GROUP], nw = genmul_windows(G::GROUP);
    const uint32_t     n = nw << w;
    void *             d_s = nullptr, *d_p = nullptr, *d_t = nullptr;
    int                rc  = K16_OK;
    auto               hip = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && !rc) {
            ctx->err = std::string(what) + ": " + hipGetErrorString(e);
            rc       = K16_ERR_HIP;
        }
    };
    hip(hipMalloc(&d_s, (size_t)n * 32), "hipMalloc(generator table scalars)");
    if (!rc) hip(hipMalloc(&d_p, (size_t)n * sizeof(typename G::Out)), "hipMalloc(generator table points)");
    if (!rc) hip(hipMalloc(&d_t, (size_t)n * G::ENTRY_WORDS * 4), "hipMalloc(generator table)");
    if (!rc) {
        hipLaunchKernelGGL(k_genmul_table_scalars, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, w, nw, (uint32_t*)d_s);
        hip(hipGetLastError(), "k_genmul_table_scalars");
    }
    // the entries by the per-point double-and-add kernel: 27 K points once per context
    if (!rc) rc = k16_synth_points_scalars(ctx, G::GROUP == 0 ? K16_G1 : K16_G2, d_s, n, d_p);
    if (!rc) {
        hipLaunchKernelGGL((k_genmul_table_pack<G>), dim3((n + 255) / 256), dim3(256), 0, ctx->stream,
                           (const typename G::Out*)d_p, n, (uint32_t*)d_t);
        hip(hipGetLastError(), "k_genmul_table_pack");
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream); // the temporaries are freed below
    hip(es, "hipStreamSynchronize(generator table)");
    if (d_s) (void)hipFree(d_s);
    if (d_p) (void)hipFree(d_p);
    if (rc) {
        if (d_t) (void)hipFree(d_t);
        return rc;
    }
    ctx->gen_table[G::GROUP] = d_t;
    return K16_OK;
}

template <class G>
int genmul_run(k16_ctx* ctx, const void* d_scalars, uint64_t n, void* d_out)
{
    constexpr unsigned W = GENMUL_W[G::GROUP], CHUNK = GENMUL_CHUNK[G::GROUP];
    int                rc = genmul_table<G>(ctx);
    if (rc) return rc;
    for (uint64_t at = 0; at < n; at += GENMUL_BATCH[G::GROUP]) {
        const uint64_t cnt     = std::min<uint64_t>(n - at, GENMUL_BATCH[G::GROUP]);
        const uint64_t n_lanes = ((cnt + CHUNK - 1) / CHUNK + 63) / 64 * 64;
        if ((rc = k16_ws_reserve(ctx, ctx->gen_scratch, (size_t)CHUNK * 4 * n_lanes * sizeof(typename G::F)))) return rc;
        hipLaunchKernelGGL((k_genmul<G, W, CHUNK>), dim3((unsigned)(n_lanes / 64)), dim3(64), 0, ctx->stream,
                           (const uint32_t*)ctx->gen_table[G::GROUP], (const uint32_t*)d_scalars + 8 * at, cnt, n_lanes,
                           (typename G::F*)ctx->gen_scratch.p, (typename G::Out*)d_out + at);
        K16_HIP(ctx, hipGetLastError());
    }
    return K16_OK;
}

// ---------------------------------------------------------------- host field helpers (canonical Montgomery Fr, bn254_field.h)
Fr fr_from_std(const uint8_t* p)
{
    Fr x;
    memcpy(x.v, p, 32);
    return to_mont(x);
}
Fr fr_small(uint32_t v)
{
    Fr x = Fr::zero();
    x.v[0] = v;
    return to_mont(x);
}
Fr fr_packed(const Fr& mont) // canonical Montgomery -> the packed R' words the kernels load
{
    Fr w;
    fr9_store(w.v, fr9_from_fr(mont));
    return w;
}
bool std_in_range(const uint8_t* p) // in [1, r)
{
    R1csFr x = r1cs_fr_load(p);
    return !r1cs_fr_is_zero(x) && !r1cs_fr_geq_r(x);
}

struct DevBufs { // freed on every way out
    std::vector<void*> p;
    ~DevBufs()
    {
        for (void* q : p)
            if (q) (void)hipFree(q);
    }
};

int setup_run(k16_ctx* ctx, const R1csFile& f, const SetupShape& sh, const uint8_t* td, uint8_t* out)
{
    const Fr tau = fr_from_std(td), alpha = fr_from_std(td + 32), beta = fr_from_std(td + 64), gamma = fr_from_std(td + 96),
             delta = fr_from_std(td + 128);
    const Fr one = Fr::one();
    // g = 5^((r - 1) / 2N), the primitive 2N-th root the prover's transforms use; omega = g^2
    uint32_t e[8];
    for (int i = 0; i < 8; i++) e[i] = FrParams::P[i];
    e[0] -= 1;
    const unsigned s = sh.log_n + 1;
    for (int i = 0; i < 8; i++) e[i] = (e[i] >> s) | (i < 7 && s < 32 ? e[i + 1] << (32 - s) : 0);
    const Fr g = fpow(fr_small(5), e), omega = fsqr(g), g_inv = finv_bgcd(g);
    Fr       tau_n = tau;
    for (unsigned k = 0; k < sh.log_n; k++) tau_n = fsqr(tau_n);
    if (fsqr(tau_n) == one) {
        ctx->err = "setup: tau^(2N) = 1 -- tau lies in the domain or in its odd coset";
        return K16_ERR_ARG;
    }
    const Fr tau_c = fmul(tau, g_inv);
    Fr       tau_cn = tau_c;
    for (unsigned k = 0; k < sh.log_n; k++) tau_cn = fsqr(tau_cn);
    const Fr n_inv = finv_bgcd(fr_small(sh.N)), z_tau = fsub(tau_n, one);
    const Fr omega_inv = finv_bgcd(omega);
    LagArgs  la0 = {fr_packed(tau), fr_packed(fmul(z_tau, n_inv)), fr_packed(omega), fr_packed(omega_inv)};
    LagArgs  la1 = {fr_packed(tau_c), fr_packed(fmul(fsub(tau_cn, one), n_inv)), fr_packed(omega), fr_packed(omega_inv)};
    MixArgs  mx  = {fr_packed(alpha), fr_packed(beta), fr_packed(finv_bgcd(gamma)), fr_packed(finv_bgcd(delta)),
                    fr_packed(fmul(z_tau, finv_bgcd(fneg(fdbl(delta)))))};

    SetupColumns cols;
    if (setup_columns_build(f, sh, &cols)) {
        ctx->err = "setup: too many terms for 32-bit entry offsets";
        return K16_ERR_ARG;
    }
    const SpmvPlan&     pl = cols.plan;
    std::vector<R1csFr> coef9(cols.coef.size());
    const R1csScale     to_r9(261); // the gathered vector is an R' value already: k * 2^261 keeps the product one
    for (size_t i = 0; i < coef9.size(); i++) coef9[i] = to_r9(cols.coef[i]);

    K16_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBufs     bufs;
    auto        dalloc = [&](size_t bytes, void** p) -> hipError_t {
        hipError_t e_ = hipMalloc(p, std::max<size_t>(bytes, 32));
        if (e_ == hipSuccess) bufs.p.push_back(*p);
        return e_;
    };
    const size_t nw = sh.n_wires, np1 = (size_t)sh.n_public + 1, N = sh.N;
    SpmvSlice*   d_slices = nullptr;
    SpmvLong*    d_longs  = nullptr;
    uint32_t *   d_rowof = nullptr, *d_cons = nullptr;
    Fr *         d_coef = nullptr, *d_lag = nullptr, *d_cols = nullptr, *d_scal = nullptr;
    void*        d_pts  = nullptr;
    // scalars, standard form: a [nw] | b [nw] | ic [np1] | c [nw - np1] | h [N] | alpha beta delta | beta gamma delta
    const size_t o_a = 0, o_b = nw, o_ic = 2 * nw, o_c = 2 * nw + np1, o_h = 3 * nw, o_hdr = 3 * nw + N, n_scal = o_hdr + 6;
    const size_t pts_bytes = std::max<size_t>(std::max<size_t>(nw * 128, N * 64), 3 * 128);
    K16_HIP(ctx, dalloc(pl.slices.size() * sizeof(SpmvSlice), (void**)&d_slices));
    K16_HIP(ctx, dalloc(pl.longs.size() * sizeof(SpmvLong), (void**)&d_longs));
    K16_HIP(ctx, dalloc(pl.row_of.size() * 4, (void**)&d_rowof));
    K16_HIP(ctx, dalloc(cols.cons.size() * 4, (void**)&d_cons));
    K16_HIP(ctx, dalloc(coef9.size() * 32, (void**)&d_coef));
    K16_HIP(ctx, dalloc(2 * N * 32, (void**)&d_lag));
    K16_HIP(ctx, dalloc(3 * nw * 32, (void**)&d_cols));
    K16_HIP(ctx, dalloc(n_scal * 32, (void**)&d_scal));
    K16_HIP(ctx, dalloc(pts_bytes, &d_pts));
    uint8_t hdr[6 * 32];
    memcpy(hdr, td + 32, 32);        // alpha
    memcpy(hdr + 32, td + 64, 32);   // beta
    memcpy(hdr + 64, td + 128, 32);  // delta
    memcpy(hdr + 96, td + 64, 32);   // beta
    memcpy(hdr + 128, td + 96, 32);  // gamma
    memcpy(hdr + 160, td + 128, 32); // delta
    // (synchronous copies from pageable memory: the vectors above stay alive until the last one has returned)
    K16_HIP(ctx, hipMemcpy(d_slices, pl.slices.data(), pl.slices.size() * sizeof(SpmvSlice), hipMemcpyHostToDevice));
    K16_HIP(ctx, hipMemcpy(d_longs, pl.longs.data(), pl.longs.size() * sizeof(SpmvLong), hipMemcpyHostToDevice));
    K16_HIP(ctx, hipMemcpy(d_rowof, pl.row_of.data(), pl.row_of.size() * 4, hipMemcpyHostToDevice));
    K16_HIP(ctx, hipMemcpy(d_cons, cols.cons.data(), cols.cons.size() * 4, hipMemcpyHostToDevice));
    K16_HIP(ctx, hipMemcpy(d_coef, coef9.data(), coef9.size() * 32, hipMemcpyHostToDevice));
    K16_HIP(ctx, hipMemcpy(d_scal + o_hdr, hdr, sizeof hdr, hipMemcpyHostToDevice));
    {
        k16_stat_scope sc(ctx, "setup_lagrange", st);
        const unsigned lanes = (unsigned)((N + LAG_CHUNK - 1) / LAG_CHUNK);
        hipLaunchKernelGGL(k_setup_lagrange, dim3((lanes + 63) / 64, 2), dim3(64), 0, st, la0, la1, sh.N, d_lag);
    }
    {
        k16_stat_scope sc(ctx, "setup_columns", st);
        const uint64_t waves = (uint64_t)pl.n_slices + pl.n_long;
        hipLaunchKernelGGL(k_setup_columns, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, d_slices, pl.n_slices, d_rowof,
                           d_longs, pl.n_long, d_cons, d_coef, d_lag, d_cols);
        const size_t most = std::max(nw, N);
        hipLaunchKernelGGL(k_setup_scalars, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, st, d_cols, sh.n_wires, sh.n_public,
                           d_lag + N, sh.N, mx, d_scal + o_a, d_scal + o_b, d_scal + o_ic, d_scal + o_c, d_scal + o_h);
    }
    K16_HIP(ctx, hipGetLastError());
    // the point sections, one after the other through d_pts
    auto section = [&](int group, size_t first, size_t n, uint8_t* dst) -> int {
        if (n == 0) return K16_OK;
        {
            k16_stat_scope sc(ctx, group == K16_G1 ? "setup_points_g1" : "setup_points_g2", st);
            const int rc = k16_generator_mul(ctx, group, d_scal + first, n, d_pts);
            if (rc) return rc;
        }
        K16_HIP(ctx, hipMemcpyAsync(dst, d_pts, n * (group == K16_G1 ? 64 : 128), hipMemcpyDeviceToHost, st));
        K16_HIP(ctx, hipStreamSynchronize(st));
        return K16_OK;
    };
    int      rc;
    uint8_t  h1[3 * 64], h2[3 * 128];
    if ((rc = section(K16_G1, o_hdr, 3, h1))) return rc;
    if ((rc = section(K16_G2, o_hdr + 3, 3, h2))) return rc;
    uint8_t* hp = out + sh.off[2] + SETUP_HEADER_INTS;
    memcpy(hp, h1, 64);              // alpha1
    memcpy(hp + 64, h1 + 64, 64);    // beta1
    memcpy(hp + 128, h2, 128);       // beta2
    memcpy(hp + 256, h2 + 128, 128); // gamma2
    memcpy(hp + 384, h1 + 128, 64);  // delta1
    memcpy(hp + 448, h2 + 256, 128); // delta2
    if ((rc = section(K16_G1, o_ic, np1, out + sh.off[3]))) return rc;
    if ((rc = section(K16_G1, o_a, nw, out + sh.off[5]))) return rc;
    if ((rc = section(K16_G1, o_b, nw, out + sh.off[6]))) return rc;
    if ((rc = section(K16_G2, o_b, nw, out + sh.off[7]))) return rc;
    if ((rc = section(K16_G1, o_c, nw - np1, out + sh.off[8]))) return rc;
    if ((rc = section(K16_G1, o_h, N, out + sh.off[9]))) return rc;
    setup_write_frame(f, sh, out);
    return K16_OK;
}

// arguments, shape and trapdoor of the three entry points; td receives the trapdoor to use
int setup_prepare(k16_ctx* ctx, k16_r1cs* r, const uint8_t* trapdoor160, const R1csFile** file, SetupShape* sh, uint8_t td[160])
{
    k16_ctx* owner = nullptr;
    k16_r1cs_view(r, &owner, file);
    if (owner != ctx) {
        ctx->err = "setup: the R1CS object lives on another context";
        return K16_ERR_ARG;
    }
    const char* why = "";
    if (setup_shape(**file, sh, &why)) {
        ctx->err = why;
        return K16_ERR_ARG;
    }
    if (trapdoor160) {
        memcpy(td, trapdoor160, 160);
        for (int k = 0; k < 5; k++)
            if (!std_in_range(td + 32 * k)) {
                ctx->err = "setup: a trapdoor value is 0 or not below r";
                return K16_ERR_ARG;
            }
        return K16_OK;
    }
    for (int k = 0; k < 5; k++) {
        do {
            if (k16_random_scalar(td + 32 * k)) {
                ctx->err = "setup: no random bytes from the OS";
                return K16_ERR_IO;
            }
        } while (!std_in_range(td + 32 * k));
    }
    return K16_OK;
}

} // namespace

extern "C" int k16_generator_mul_info(int group, unsigned* window_bits, unsigned* n_windows)
{
    if (group != K16_G1 && group != K16_G2) return K16_ERR_ARG;
    const int g = group == K16_G1 ? 0 : 1;
    if (window_bits) *window_bits = GENMUL_W[g];
    if (n_windows) *n_windows = genmul_windows(g);
    return K16_OK;
}

extern "C" int k16_generator_mul(k16_ctx* ctx, int group, const void* d_scalars, uint64_t n, void* d_out_affine)
{
    return k16_guard(ctx, [&]() -> int {
    if (!ctx || !d_scalars || !d_out_affine || (group != K16_G1 && group != K16_G2)) return K16_ERR_ARG;
    if (n == 0) return K16_OK;
    K16_HIP(ctx, hipSetDevice(ctx->device));
    return group == K16_G1 ? genmul_run<GenG1>(ctx, d_scalars, n, d_out_affine) : genmul_run<GenG2>(ctx, d_scalars, n, d_out_affine);
    });
}

extern "C" int k16_r1cs_setup_size(const k16_r1cs* r, uint64_t* zkey_bytes)
{
    return k16_guard(nullptr, [&]() -> int {
    if (!r || !zkey_bytes) return K16_ERR_ARG;
    *zkey_bytes = 0;
    k16_ctx*        ctx  = nullptr;
    const R1csFile* file = nullptr;
    k16_r1cs_view(r, &ctx, &file);
    SetupShape  sh;
    const char* why = "";
    if (setup_shape(*file, &sh, &why)) {
        ctx->err = why;
        return K16_ERR_ARG;
    }
    *zkey_bytes = sh.total;
    return K16_OK;
    });
}

extern "C" int k16_r1cs_setup(k16_ctx* ctx, k16_r1cs* r, const uint8_t* trapdoor160, void* out_zkey, size_t cap, size_t* out_size)
{
    return k16_guard(ctx, [&]() -> int {
    if (!ctx || !r || !out_size) return K16_ERR_ARG;
    *out_size = 0;
    const R1csFile* file = nullptr;
    SetupShape      sh;
    uint8_t         td[160];
    int             rc = setup_prepare(ctx, r, trapdoor160, &file, &sh, td);
    if (rc) return rc;
    *out_size = (size_t)sh.total;
    if (!out_zkey || cap < sh.total) {
        ctx->err = "setup: the buffer is smaller than the key";
        return K16_ERR_BUFFER;
    }
    rc = setup_run(ctx, *file, sh, td, (uint8_t*)out_zkey);
    if (rc) (void)hipStreamSynchronize(ctx->stream); // nothing of the set-up stays in flight
    return rc;
    });
}

extern "C" int k16_r1cs_setup_file(k16_ctx* ctx, k16_r1cs* r, const uint8_t* trapdoor160, const char* zkey_path)
{
    return k16_guard(ctx, [&]() -> int {
    if (!ctx || !r || !zkey_path) return K16_ERR_ARG;
    const R1csFile* file = nullptr;
    SetupShape      sh;
    uint8_t         td[160];
    int             rc = setup_prepare(ctx, r, trapdoor160, &file, &sh, td);
    if (rc) return rc;
    std::vector<uint8_t> key((size_t)sh.total);
    rc = setup_run(ctx, *file, sh, td, key.data());
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    // written under a temporary name beside the target and renamed: no partial file under zkey_path
    const std::string tmp = std::string(zkey_path) + ".tmp." + std::to_string((long)getpid());
    FILE*             fp  = fopen(tmp.c_str(), "wb");
    bool              ok  = fp != nullptr;
    if (ok) ok = fwrite(key.data(), 1, key.size(), fp) == key.size();
    if (fp) ok = (fclose(fp) == 0) && ok;
    if (ok) ok = rename(tmp.c_str(), zkey_path) == 0;
    if (!ok) {
        (void)remove(tmp.c_str());
        ctx->err = std::string("setup: cannot write ") + zkey_path;
        return K16_ERR_IO;
    }
    return K16_OK;
    });
}
