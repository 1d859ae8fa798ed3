// Host-only guard of the filters' setup arithmetic: pairb_desc_of, recip_grid_of and recip_grids_of of
// kss_internal.hpp on heap arrays of exactly the size they may read -- one segment, many segments, a zero-length segment, the row
// cap, the 32-bit limits, and boxes that are a point, a plane, not finite or empty.  Needs no GPU; meant for the host sanitizers:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -I kss-icp_amd/csrc tools/recip_host_check.hip -o tools/recip_host_check && tools/recip_host_check      # prints "fails: 0"
#include "kss_internal.hpp"

#include <array>
#include <cstdio>
#include <memory>

using namespace kss;

static int fails = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

// the descriptors of segments of the given source and target counts, through offsets that start at `lead`
static void check_desc(const std::vector<int64_t>& ns, const std::vector<int64_t>& nt, int64_t lead) {
    const int nseg = (int)ns.size();
    std::unique_ptr<int64_t[]> off(new int64_t[nseg + 1]), toff(new int64_t[nseg + 1]);   // exactly nseg + 1 entries each
    off[0] = lead; toff[0] = 0;
    for (int i = 0; i < nseg; ++i) { off[i + 1] = off[i] + ns[i]; toff[i + 1] = toff[i] + nt[i]; }
    std::vector<PairbDesc> desc(3);   // (a vector that held something else before)
    int64_t rows = -1;
    EXPECT(pairb_desc_of(off.get(), toff.get(), nseg, desc, rows));
    EXPECT((int)desc.size() == nseg);
    int64_t row = 0;
    for (int i = 0; i < nseg; ++i) {
        const PairbDesc& d = desc[i];
        EXPECT(d.src_base == off[i] && d.ns == ns[i] && d.tgt_off == toff[i] && d.nt == nt[i] && d.overlap == 1.0);
        EXPECT(d.row_base == row && d.nrows == stream_blocks(ns[i]) && d.nrows >= 1 && d.nrows <= 2048);
        EXPECT((int64_t)d.nrows * 256 >= std::min<int64_t>(ns[i], 2048 * 256));
        row += d.nrows;
    }
    EXPECT(rows == row);
}

// the grids of np pairs from `split` partials each; the partials of pair p spread the box b[p] = {min xyz, max xyz} over the
// partials, the rest of them empty ({+inf, -inf})
static void check_grids(const std::vector<std::array<float, 6>>& b, const std::vector<int64_t>& ns, int split) {
    const size_t np = b.size();
    std::unique_ptr<float[]> box(new float[np * split * 6]);   // exactly np * split partials
    for (size_t p = 0; p < np; ++p)
        for (int s = 0; s < split; ++s)
            for (int k = 0; k < 6; ++k) {
                const bool here = s == (int)((p + k) % split);   // every bound sits in one partial, not all in the same
                box[(p * split + s) * 6 + k] = here ? b[p][k] : (k < 3 ? INFINITY : -INFINITY);
            }
    std::vector<PairbDesc> desc(np);
    for (size_t p = 0; p < np; ++p) { desc[p] = PairbDesc(); desc[p].ns = ns[p]; }
    std::vector<RecipPairDev> grids;
    const int64_t cells = recip_grids_of(box.get(), split, desc, grids);
    EXPECT(grids.size() == np);
    int64_t sum = 0;
    for (size_t p = 0; p < np; ++p) {
        const RecipGrid g = grids[p].g, want = recip_grid_of(b[p].data(), b[p].data() + 3, ns[p]);
        EXPECT(grids[p].cell_base == sum);
        EXPECT(g.gx == want.gx && g.gy == want.gy && g.gz == want.gz && g.inv_h == want.inv_h && g.ox == want.ox && g.oy == want.oy && g.oz == want.oz);
        EXPECT(g.gx >= 1 && g.gx <= RECIP_GMAX && g.gy >= 1 && g.gy <= RECIP_GMAX && g.gz >= 1 && g.gz <= RECIP_GMAX);
        EXPECT(std::isfinite(g.inv_h) && g.inv_h >= 0.0f && std::isfinite(g.ox) && std::isfinite(g.oy) && std::isfinite(g.oz));
        EXPECT(recip_cells(g) <= 2 * (int64_t)RECIP_GMAX * RECIP_GMAX * RECIP_GMAX);
        sum += recip_cells(g);
    }
    EXPECT(cells == sum);
}

int main() {
    // one segment (the single pair's descriptor: src_base 0, tgt_off 0, row_base 0, nrows stream_blocks(n)), many, offsets not from 0
    check_desc({257}, {190}, 0);
    check_desc({1}, {1}, 0);
    check_desc({1, 64, 65, 257, 4096, 300}, {1, 48, 40, 190, 3000, 220}, 0);
    check_desc({1, 64, 65, 257, 4096, 300}, {1, 48, 40, 190, 3000, 220}, 5);
    // a zero-length segment keeps one row and no source; the row cap
    check_desc({300, 0, 7}, {5, 0, 9}, 0);
    check_desc({2048 * 256 + 257, 3}, {300, 300}, 0);
    EXPECT(stream_blocks(0) == 1 && stream_blocks(256) == 1 && stream_blocks(257) == 2 && stream_blocks(2048 * 256 + 257) == 2048);
    {   // the limits: too many targets, too many rows
        std::vector<PairbDesc> desc;
        int64_t rows = 0;
        const int64_t off[3] = {0, 10, 20}, big_t[3] = {0, 0x7fff0000ll, 0x7fff0001ll}, ok_t[3] = {0, 0x7fff0000ll - 1, 0x7fff0000ll};
        EXPECT(!pairb_desc_of(off, big_t, 2, desc, rows));
        EXPECT(pairb_desc_of(off, ok_t, 2, desc, rows) && rows == 2);
        const int many = 1100000;   // 1.1e6 segments of 2048 rows each pass 0x7fff0000 rows
        std::unique_ptr<int64_t[]> o(new int64_t[many + 1]), t(new int64_t[many + 1]);
        for (int i = 0; i <= many; ++i) { o[i] = (int64_t)i * 2048 * 256; t[i] = i; }
        EXPECT(!pairb_desc_of(o.get(), t.get(), many, desc, rows));
    }
    // boxes: a volume, a point, a plane, a line, one non-finite bound, NaN, an empty box (no target at all), a huge and a tiny one
    const float inf = INFINITY, nan = NAN;
    const std::vector<std::array<float, 6>> boxes = {
        {-1, -1, -1, 1, 1, 1}, {0.3f, -0.2f, 0.1f, 0.3f, -0.2f, 0.1f}, {-1, -1, 0, 1, 1, 0}, {-1, 0.25f, -0.5f, 1, 0.25f, -0.5f},
        {-1, -1, -1, 1, inf, 1}, {-1, nan, -1, 1, 1, 1}, {inf, inf, inf, -inf, -inf, -inf}, {-3e38f, -3e38f, -3e38f, 3e38f, 3e38f, 3e38f},
        {1, 1, 1, 1.0000001f, 1, 1}, {0, 0, 0, 1e-44f, 1e-44f, 1e-44f}, {-0.0f, 0, 0, 0.0f, 1, 1}};
    for (const int64_t n : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)257, (int64_t)100000, (int64_t)0x7fff0000ll})
        for (const int split : {1, 3, 64, 256})
            check_grids(boxes, std::vector<int64_t>(boxes.size(), n), split);
    check_grids({boxes[0]}, {100000}, 1);                       // one pair, one partial
    check_grids({boxes[1], boxes[0], boxes[6]}, {5, 70000, 9}, 2);
    {   // one cell for whatever is no box; the cell total's limit
        const RecipGrid g = recip_grid_of(boxes[5].data(), boxes[5].data() + 3, 1000);
        EXPECT(g.gx == 1 && g.gy == 1 && g.gz == 1 && g.inv_h == 0.0f);
        const RecipGrid full = recip_grid_of(boxes[0].data(), boxes[0].data() + 3, 100000);
        EXPECT(recip_cells(full) > 16384 && recip_cells(full) <= 2 * RECIP_CELLS);
        const size_t np = (size_t)(PAIRB_INDEX_MAX / recip_cells(full)) + 2;
        std::unique_ptr<float[]> box(new float[np * 6]);
        for (size_t p = 0; p < np; ++p)
            for (int k = 0; k < 6; ++k) box[p * 6 + k] = boxes[0][k];
        std::vector<PairbDesc> desc(np);
        for (PairbDesc& d : desc) { d = PairbDesc(); d.ns = 100000; }
        std::vector<RecipPairDev> grids;
        EXPECT(recip_grids_of(box.get(), 1, desc, grids) == -1);
    }
    std::printf("fails: %d\n", fails);
    return fails != 0;
}
