// tests/cpp/chain_spmv_model.cpp -- what k_spmv (prover.hip) leaves in HBM for a given .zkey and .wtns, computed on the host
// with the device's own arithmetic: spmv_plan.h lays the rows out as k16_prover_create does, the coefficients are converted
// the same way (ten modular doublings of the file's value), and every row is accumulated in the kernel's order with the
// functions of bn254_fq9.h (they are __host__ __device__) -- slices lane by lane over slice.len entries including the
// (wire 0, coefficient 0) padding, long rows as 64 strided lanes and the xor-shuffle reduction.
// Prints one line per non-empty row:   <row id> <S|L> <p> <q> <packed value, 64 hex digits, most significant first>
//   S (slice row): p = entries the lane walks (the slice's length), q = the row's own entries
//   L (long row):  p = lanes that hold at least one entry, q = most entries in one lane
// Row id = (matrix == 0 ? 0 : N) + constraint.  tests/test_chain_directed_host.py reads the representatives from it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "bn254_curve.h"
#include "bn254_fq9.h"
#include "spmv_plan.h"
using namespace k16;

static std::vector<uint8_t> slurp(const char* path)
{
    std::vector<uint8_t> v;
    FILE*                f = fopen(path, "rb");
    if (!f) return v;
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t)n);
    if (fread(v.data(), 1, (size_t)n, f) != (size_t)n) v.clear();
    fclose(f);
    return v;
}
// iden3 container: magic[4] version[4] n_sections[4] { type[4] size[8] payload }*
static const uint8_t* section(const std::vector<uint8_t>& f, uint32_t type, uint64_t* size)
{
    size_t at = 12;
    while (at + 12 <= f.size()) {
        uint32_t t;
        uint64_t n;
        memcpy(&t, &f[at], 4);
        memcpy(&n, &f[at + 4], 8);
        if (at + 12 + n > f.size()) return nullptr;
        if (t == type) {
            *size = n;
            return &f[at + 12];
        }
        at += 12 + n;
    }
    return nullptr;
}
static Fr9 ld9(const uint8_t* p)
{
    uint32_t w[8];
    memcpy(w, p, 32);
    return fr9_load(w);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const std::vector<uint8_t> zk = slurp(argv[1]), wt = slurp(argv[2]);
    uint64_t       hs = 0, cs = 0, ws = 0;
    const uint8_t *h = section(zk, 2, &hs), *c4 = section(zk, 4, &cs), *w2 = section(wt, 2, &ws);
    if (!h || !c4 || !w2 || hs < 4 + 32 + 4 + 32 + 12 || cs < 4) return 3;
    uint32_t n_vars, N, n_coefs;
    memcpy(&n_vars, h + 72, 4);
    memcpy(&N, h + 80, 4);
    memcpy(&n_coefs, c4, 4);
    if (cs < 4 + (uint64_t)n_coefs * 44 || ws < (uint64_t)n_vars * 32) return 3;
    const uint8_t* cf = c4 + 4;
    SpmvPlan       plan;
    if (spmv_plan_build(cf, n_coefs, N, n_vars, &plan)) return 4;
    // entries as k16_prover_create fills them
    std::vector<uint32_t> wire(plan.n_entries ? plan.n_entries : 1, 0);
    std::vector<uint8_t>  vals((plan.n_entries ? plan.n_entries : 1) * 32, 0);
    std::vector<uint32_t> len(2 * (size_t)N, 0);
    for (uint64_t i = 0; i < n_coefs; i++) {
        const size_t pos = plan.pos_of[i];
        uint32_t     m, c;
        memcpy(&m, cf + i * 44, 4);
        memcpy(&c, cf + i * 44 + 4, 4);
        memcpy(&wire[pos], cf + i * 44 + 8, 4);
        len[(m == 0 ? 0 : N) + c]++;
        Fr cv;
        memcpy(cv.v, cf + i * 44 + 12, 32);
        for (int d = 0; d < 10; d++) cv = fdbl(cv);
        memcpy(&vals[pos * 32], cv.v, 32);
    }
    // k_spmv's term(): the single-limb product for a wire below 256 (the n16 word), the full one otherwise
    auto term = [&](uint32_t e) -> Fr9 {
        const uint8_t* w = w2 + (size_t)wire[e] * 32;
        bool           wide = false;
        for (int i = 1; i < 32; i++) wide = wide || w[i];
        if (!wide) return fmul9_small_t<Fr9C>(ld9(&vals[(size_t)e * 32]), w[0]);
        return frmul9(ld9(w), ld9(&vals[(size_t)e * 32]));
    };
    auto print = [&](uint32_t row, char kind, uint32_t p, uint32_t q, const Fr9& acc) {
        uint32_t w[8];
        fr9_store(w, acc);
        printf("%u %c %u %u ", row, kind, p, q);
        for (int i = 7; i >= 0; i--) printf("%08x", w[i]);
        printf("\n");
    };
    printf("N %u slices %u long %u\n", N, plan.n_slices, plan.n_long);
    for (uint32_t s = 0; s < plan.n_slices; s++) {
        const SpmvSlice sl = plan.slices[s];
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t row = plan.row_of[64ull * s + lane];
            if (row == 0xffffffffu || len[row] == 0) continue;
            Fr9 acc = fq9_zero();
            for (uint32_t k = 0; k < sl.len; k++) acc = fradd9(acc, term(sl.off + (k << 6) + lane));
            print(row, 'S', sl.len, len[row], acc);
        }
    }
    for (uint32_t k = 0; k < plan.n_long; k++) {
        const SpmvLong L = plan.longs[k];
        Fr9            acc[64];
        uint32_t       lanes = 0, most = 0;
        for (uint32_t lane = 0; lane < 64; lane++) {
            acc[lane]  = fq9_zero();
            uint32_t n = 0;
            for (uint32_t j = lane; j < L.len; j += 64, n++) acc[lane] = fradd9(acc[lane], term(L.off + j));
            lanes += n ? 1 : 0;
            most = n > most ? n : most;
        }
        for (int d = 32; d >= 1; d >>= 1) {
            Fr9 nxt[64];
            for (int lane = 0; lane < 64; lane++) nxt[lane] = fradd9(acc[lane], acc[lane ^ d]);
            memcpy(acc, nxt, sizeof(acc));
        }
        print(L.row, 'L', lanes, most, acc[0]);
    }
    return 0;
}
