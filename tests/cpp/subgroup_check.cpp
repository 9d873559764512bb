// tests/cpp/subgroup_check.cpp -- runs the point checks of keyless-zk-proofs_amd/csrc/bn254_points.h (the same
// __host__ __device__ sequence the kernels of points_check.hip compile) on the CPU.
//   subgroup_check g2 IN OUT   IN: n x 128 B affine Montgomery twist points; OUT: n x 2 statuses, the test run on the
//                              canonical field (Fq2) and on the radix-2^29 field (Fq2n)
//   subgroup_check g1 IN OUT   IN: n x 64 B; OUT: n statuses
// Used by tests/test_subgroup_host.py to compare with the definitional test [r] Q = O without a GPU.
#include <cstdio>
#include <cstring>
#include <vector>
#include "bn254_pairing.h"
#include "bn254_points.h"
using namespace k16;

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    const bool g2 = strcmp(argv[1], "g2") == 0;
    FILE*      fi = fopen(argv[2], "rb");
    if (!fi) return 2;
    std::vector<unsigned char> in;
    unsigned char              buf[4096];
    size_t                     got;
    while ((got = fread(buf, 1, sizeof buf, fi)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(fi);
    PairConsts K;
    pairing_consts_init(&K);
    const G2Consts       G{K.twist_b, K.twqx, K.twqy};
    const size_t         psz = g2 ? 128 : 64, n = in.size() / psz;
    std::vector<uint8_t> out;
    for (size_t i = 0; i < n; i++) {
        if (g2) {
            G2Aff b;
            memcpy(&b, &in[i * psz], sizeof b);
            out.push_back(g2_point_status<Fq2>(b, G));
            out.push_back(g2_point_status<Fq2n>(b, G));
        } else {
            G1Aff a;
            memcpy(&a, &in[i * psz], sizeof a);
            out.push_back(g1_point_status(a));
        }
    }
    FILE* fo = fopen(argv[3], "wb");
    if (!fo) return 2;
    fwrite(out.data(), 1, out.size(), fo);
    fclose(fo);
    printf("OK %zu\n", n);
    return 0;
}
