// Host-only guard of the host <-> device hand-over: the host functions of kss_handover.hpp on heap blocks of
// exactly the size they may touch (gate records 16-byte aligned), against plain C++ restatements of what the device does on the
// other side -- the kernels' acceptance test of a gate record, pub_put's result slot, res_store_exit_flag's flag.  Needs no GPU;
// meant for the host sanitizers:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -I kss-icp_amd/csrc tools/handover_host_check.hip -o tools/handover_host_check && tools/handover_host_check      # prints "fails: 0"
#include "kss_handover.hpp"

#include <cstdio>
#include <cstdlib>
#include <memory>

using namespace kss;

static int fails = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

struct FreeIt { void operator()(void* p) const { std::free(p); } };
static std::unique_ptr<unsigned, FreeIt> gate_block() { return std::unique_ptr<unsigned, FreeIt>((unsigned*)std::aligned_alloc(16, 80)); }   // five granules, no more

// the device's acceptance test: granule g is taken when v.w - kss_mix3(v.x, v.y, v.z) == stamp; returns how many of the five pass
// (bad: the last one that does not) and the 15 words as the kernels copy them to LDS
static int device_accepts(const unsigned* rec, unsigned stamp, unsigned out[15], int* bad = nullptr) {
    int ok = 0;
    for (int g = 0; g < 5; ++g) {
        const unsigned x = rec[4 * g], y = rec[4 * g + 1], z = rec[4 * g + 2], w = rec[4 * g + 3];
        if (w - kss_mix3(x, y, z) == stamp) ++ok; else if (bad) *bad = g;
        out[3 * g] = x; out[3 * g + 1] = y; out[3 * g + 2] = z;
    }
    return ok;
}
// pub_put (kss_device.hpp) and res_store_exit_flag as the device writes them
static void device_pub_put(unsigned long long* pub, int slot, double v, unsigned long long seq) {
    unsigned long long b;
    std::memcpy(&b, &v, sizeof b);
    const unsigned x = (unsigned)b, y = (unsigned)(b >> 32), z = (unsigned)seq, w = kss_mix3(x, y, z);
    pub[2 * slot] = b;
    pub[2 * slot + 1] = (unsigned long long)z | ((unsigned long long)w << 32);
}
static void device_exit_flag(unsigned long long* flags, int pair, unsigned tag, unsigned note) {
    const unsigned w = kss_mix3(tag, (unsigned)pair, note);
    flags[2 * pair] = (unsigned long long)tag | ((unsigned long long)(unsigned)pair << 32);
    flags[2 * pair + 1] = (unsigned long long)note | ((unsigned long long)w << 32);
}

static unsigned rnd_state = 12345u;
static unsigned rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state ^ (rnd_state >> 13); }

static void check_gate(unsigned stamp) {
    auto rec = gate_block();
    unsigned w[15], got[15];
    for (unsigned& x : w) x = rnd();
    gate_record_store(rec.get(), w, stamp, false);
    EXPECT(device_accepts(rec.get(), stamp, got) == 5 && std::memcmp(got, w, sizeof w) == 0);
    EXPECT(device_accepts(rec.get(), stamp + 1u, got) == 0 && device_accepts(rec.get(), stamp - 1u, got) == 0);
    // the altered form: exactly one granule fails, one that carries transform words
    for (unsigned& x : w) x = rnd();
    int bad = -1;
    gate_record_write(rec.get(), w, stamp, true);
    EXPECT(device_accepts(rec.get(), stamp, got, &bad) == 4 && bad == GATE_TORN_GRANULE && 3 * bad + 2 < 12);
    // ... and the test hook's store ends with the right record
    gate_record_store(rec.get(), w, stamp, true);
    EXPECT(device_accepts(rec.get(), stamp, got) == 5 && std::memcmp(got, w, sizeof w) == 0);
}

int main() {
    // ---- gate records: the single pair's stamps (1 .. 0x7fffffff - 1) and the resident engines' (launch * 4096 + pass) ----
    for (const unsigned stamp : {1u, 2u, 0x7fffffffu - 1u, 4096u + 1u, 500000u * 4096u + 4002u, 500000u * 4096u + 4095u}) check_gate(stamp);
    {   // a stop order is accepted under `any` and not under `expect`; a record of launch n is nothing to launch n + 1
        auto rec = gate_block();
        unsigned w[15] = {0}, got[15];
        w[12] = 1u; w[14] = 2u;
        for (const unsigned launch : {1u, 77u, 499999u, 500000u}) {
            const unsigned stamp0 = launch * 4096u, next0 = (launch % 500000u + 1u) * 4096u;
            gate_record_store(rec.get(), w, stamp0 + RES_STAMP_ANY, false);
            EXPECT(device_accepts(rec.get(), stamp0 + RES_STAMP_ANY, got) == 5 && got[14] == 2u);
            for (unsigned k = 1; k <= 4002u; ++k) EXPECT(device_accepts(rec.get(), stamp0 + k, got) == 0);
            EXPECT(device_accepts(rec.get(), next0 + RES_STAMP_ANY, got) == 0);
            for (const unsigned k : {1u, 2u, 21u, 4002u}) {
                gate_record_store(rec.get(), w, stamp0 + k, false);
                EXPECT(device_accepts(rec.get(), stamp0 + k, got) == 5 && device_accepts(rec.get(), stamp0 + RES_STAMP_ANY, got) == 0);
                EXPECT(device_accepts(rec.get(), next0 + k, got) == 0 && device_accepts(rec.get(), next0 + RES_STAMP_ANY, got) == 0);
            }
        }
    }
    // ---- result slots ----
    for (const unsigned long long want : {1ull, 41ull, 0xffffffffull, 0x100000000ull + 7ull, 0x7fffffff00000003ull}) {
        const int n = 20;
        std::unique_ptr<unsigned long long[]> sl(new unsigned long long[2 * n]);   // exactly n slots
        std::unique_ptr<double[]> out(new double[n]), val(new double[n]);
        for (int k = 0; k < n; ++k) { val[k] = (double)(int)rnd() * 1e-3 + k; device_pub_put(sl.get(), k, val[k], want); }
        EXPECT(slots_collect(sl.get(), n, want, out.get()) && std::memcmp(out.get(), val.get(), n * sizeof(double)) == 0);
        EXPECT(slots_collect(sl.get(), n, (want & 0xffffffffull) | 0x500000000ull, out.get()));   // (the low word is what is compared)
        EXPECT(!slots_collect(sl.get(), n, want + 1, out.get()) && !slots_collect(sl.get(), n, want - 1, out.get()));
        EXPECT(slots_collect(sl.get(), 1, want, out.get()));
        for (const int k : {0, 7, n - 1})
            for (const int bit : {0, 31, 32, 52, 63}) {   // one bit of the value flipped
                sl[2 * k] ^= 1ull << bit;
                EXPECT(!slots_collect(sl.get(), n, want, out.get()) && slots_collect(sl.get(), k, want, out.get()));
                sl[2 * k] ^= 1ull << bit;
            }
        {   // the value of one write under the seq word of another: the next launch's, what a torn read would see
            const unsigned long long keep0 = sl[2 * 3], keep1 = sl[2 * 3 + 1];
            device_pub_put(sl.get(), 3, val[3] + 1.0, want + 1);
            sl[2 * 3] = keep0;
            EXPECT(!slots_collect(sl.get(), n, want + 1, out.get()) && !slots_collect(sl.get(), n, want, out.get()));
            device_pub_put(sl.get(), 3, val[3] + 1.0, want + 1);
            sl[2 * 3 + 1] = keep1;
            EXPECT(!slots_collect(sl.get(), n, want, out.get()));
            sl[2 * 3] = keep0;
            EXPECT(slots_collect(sl.get(), n, want, out.get()));
        }
    }
    // ---- exit flags ----
    {
        const int np = 6;
        std::unique_ptr<unsigned long long[]> fl(new unsigned long long[2 * np]);   // exactly np flags
        for (int i = 0; i < 2 * np; ++i) fl[i] = 0;
        const unsigned tag = 77u * 4096u;
        unsigned note = 99u;
        for (int p = 0; p < np; ++p) EXPECT(!exit_flag_read(fl.get(), p, tag, &note) && !exit_flag_read(fl.get(), p, 0u, nullptr) && note == 99u);
        for (int p = 0; p < np; ++p) device_exit_flag(fl.get(), p, tag, 1000u + (unsigned)p);
        for (int p = 0; p < np; ++p) {
            EXPECT(exit_flag_read(fl.get(), p, tag, &note) && note == 1000u + (unsigned)p && exit_flag_read(fl.get(), p, tag, nullptr));
            EXPECT(!exit_flag_read(fl.get(), p, tag + 1u, &note) && note == 1000u + (unsigned)p);   // the second launch's tag
        }
        // a flag that names another pair, a note that does not fit the check word, a check word that does not fit
        const unsigned long long k0 = fl[2 * 2], k1 = fl[2 * 2 + 1];
        fl[2 * 2] = fl[2 * 3];
        EXPECT(!exit_flag_read(fl.get(), 2, tag, nullptr));
        fl[2 * 2] = k0; fl[2 * 2 + 1] = k1 ^ 1ull;
        EXPECT(!exit_flag_read(fl.get(), 2, tag, nullptr));
        fl[2 * 2 + 1] = k1 ^ (1ull << 40);
        EXPECT(!exit_flag_read(fl.get(), 2, tag, nullptr));
        fl[2 * 2 + 1] = k1;
        EXPECT(exit_flag_read(fl.get(), 2, tag, &note) && note == 1002u);
        device_exit_flag(fl.get(), 2, tag + 1u, 5u);
        EXPECT(!exit_flag_read(fl.get(), 2, tag, nullptr) && exit_flag_read(fl.get(), 2, tag + 1u, &note) && note == 5u);
    }
    std::printf("fails: %d\n", fails);
    return fails != 0;
}
