// Host-only guard of the pair metrics' offset arithmetic: pair_check and pair_rebase over the batch shapes of
// tests/test_gpu_pair_args.py (two pairs, 8 x 7 and 5 x 6, first offset zero and non-zero, with and without normals) on heap arrays of
// exactly the packed size, every slice read through the rebased pointers and offsets.  Needs no GPU; meant for the host sanitizers:
//   cd kss-icp_amd && make && cd ../tools
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -I ../kss-icp_amd/csrc -I ../include -c pair_rebase_check.hip -o pair_rebase_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined pair_rebase_check.o $(ls ../kss-icp_amd/lib/*.o | grep -v kss_api.o) \
//         -ldl -pthread -o pair_rebase_check && ./pair_rebase_check        # prints the three refusals and "fails: 0"
#include "../kss-icp_amd/csrc/kss_api.hip"

#include <cstdio>
#include <memory>

static double touch(const float* p, int64_t n) {   // reads every float of n points: out of bounds shows under ASan
    double s = 0;
    for (int64_t i = 0; i < 3 * n; ++i) s += p[i];
    return s;
}

int main() {
    using namespace kss;
    kss_ctx* c = new kss_ctx();
    kss_icp_params p;
    kss_icp_default_params(&p);
    kss_icp_result res[2];
    int fails = 0;
    for (int lead = 0; lead <= 17; lead += 17) {
        const int64_t so[3] = {lead, lead + 8, lead + 13}, to[3] = {lead / 2, lead / 2 + 7, lead / 2 + 13};
        // heap arrays of exactly the packed size: one float past the end is a report
        std::unique_ptr<float[]> src(new float[3 * so[2]]()), tgt(new float[3 * to[2]]()), snr(new float[3 * so[2]]()), tnr(new float[3 * to[2]]());
        for (int with_nrm = 0; with_nrm < 2; ++with_nrm) {
            PairClouds P = many_pairs(src.get(), so, with_nrm ? snr.get() : nullptr, tgt.get(), to, with_nrm ? tnr.get() : nullptr, 2);
            if (pair_check(c, "t", P, &p, res, "x") != KSS_OK) { std::printf("check failed: %s\n", c->err.c_str()); ++fails; }
            pair_rebase(P);
            if (P.src != src.get() + 3 * lead || P.tgt != tgt.get() + 3 * (lead / 2)) ++fails;
            if (P.src_off[0] != 0 || P.src_off[1] != 8 || P.src_off[2] != 13 || P.tgt_off[0] != 0 || P.tgt_off[1] != 7 || P.tgt_off[2] != 13) ++fails;
            if (P.ns != 13 || P.nt != 13) ++fails;
            double s = touch(P.src, P.ns) + touch(P.tgt, P.nt);
            for (int i = 0; i < 2; ++i) s += touch(P.src + 3 * P.src_off[i], P.src_off[i + 1] - P.src_off[i]) + touch(P.tgt + 3 * P.tgt_off[i], P.tgt_off[i + 1] - P.tgt_off[i]);
            if (with_nrm) s += touch(P.snrm, P.ns) + touch(P.tnrm, P.nt);
            else if (P.snrm || P.tnrm) ++fails;
            if (s != 0) ++fails;
        }
        // one pair: nothing moves
        PairClouds Q = one_pair(src.get(), 8, nullptr, tgt.get(), 7, tnr.get());
        pair_rebase(Q);
        if (Q.src != src.get() || Q.tnrm != tnr.get() || Q.ns != 8 || Q.nt != 7) ++fails;
    }
    // the faults of the shape that pair_check must refuse before pair_rebase reads an offset
    const int64_t empty[3] = {0, 8, 8}, big[3] = {0, 0x7fff0001ll, 0x7fff0006ll}, ok[3] = {0, 7, 13};
    float one[3] = {0, 0, 0};
    for (const int64_t* off : {empty, big}) {
        PairClouds P = many_pairs(one, off, nullptr, one, ok, nullptr, 2);
        if (pair_check(c, "t", P, &p, res, "x") != KSS_ERR_ARG) ++fails;
        std::printf("refused: %s\n", c->err.c_str());
    }
    PairClouds N = many_pairs(one, nullptr, nullptr, one, ok, nullptr, 2);
    if (pair_check(c, "t", N, &p, res, "x") != KSS_ERR_ARG) ++fails;
    std::printf("refused: %s\nfails: %d\n", c->err.c_str(), fails);
    delete c;
    return fails != 0;
}
