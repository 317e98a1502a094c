// plane_layout.cpp -- the LDS layouts of the per-plane matrix loop (hz_firmm2.h, kPlane; the index maps are
// hz_firmm2_plan.h's plane_piece, plane_a_offset, plane_b_offset, tile_stride) under AddressSanitizer +
// UndefinedBehaviorSanitizer.  Built by tests/test_plane_layout.py:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I go-sdr_amd/csrc -I include
//         tests/host/plane_layout.cpp -o plane_layout
//   * the staging permutation T[f][E][part][pl] -> P[plane][E][part] is a bijection of the table's 8 ne digit pieces and
//     leaves the pieces behind them (constant term, step factors) alone;
//   * every (plane, entry, part) lies where the loop's address formula reads it, inside the table;
//   * an LDS bank model -- ds_read_b128 served in four groups of sixteen lanes, 64 banks of 4 bytes, equal addresses
//     broadcast, N different addresses on a bank N cycles -- gives 4 cycles, the conflict-free figure, for each of the
//     loop's eight reads on every pair and column block at the shipped tile stride, and 8 for the layouts the loop had
//     before (T's order for A, 144-byte tiles for B): a model that could not tell them apart would fail here;
//   * the LDS of the largest geometry the per-plane instantiation accepts fits a compute unit's 160 KiB.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <vector>

#include "hz_firmm2_plan.h"

using namespace hz::mm2;

#define REQUIRE(c)                                                              \
    do {                                                                        \
        if (!(c)) {                                                             \
            fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                                            \
        }                                                                       \
    } while (0)

// ds_read_b128's lane groups (one LDS cycle each when conflict-free): {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and
// the same + 32
static const int kGroups[4][16] = {
    {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
    {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63},
};

// LDS-array cycles of one lane group: 16 bytes per lane at byte addresses addr[], `banks` banks of 4 bytes
static int group_cycles(const int (&addr)[64], const int *lanes, int n_lanes, int banks) {
    std::set<int> on_bank[64];
    for (int k = 0; k < n_lanes; k++) {
        const int a = addr[lanes[k]];
        REQUIRE(a >= 0 && a % 16 == 0);
        for (int w = 0; w < 4; w++) on_bank[(a / 4 + w) % banks].insert(a / 4 + w);
    }
    size_t worst = 0;
    for (const auto &b : on_bank) worst = b.size() > worst ? b.size() : worst;
    return (int)worst;
}
// ... of a ds_read_b128
static int lds_cycles(const int (&addr)[64]) {
    int total = 0;
    for (const auto &grp : kGroups) total += group_cycles(addr, grp, 16, 64);
    return total;
}
// ... of a ds_write_b128: eight groups of eight consecutive lanes, bank (a / 4) mod 32 -- 8 cycles when conflict-free
static int lds_write_cycles(const int (&addr)[64]) {
    int total = 0;
    for (int g = 0; g < 8; g++) {
        int lanes[8];
        for (int k = 0; k < 8; k++) lanes[k] = 8 * g + k;
        total += group_cycles(addr, lanes, 8, 32);
    }
    return total;
}

int main() {
    constexpr int D = 8;
    long long checked = 0;

    // ---- the staging permutation, for the per-plane geometry and a few others --------------------------------------
    for (int ne : {152, 24, 40, 41, 87, 200}) {
        const int tp = (int)((table_bytes(ne) + 15) / 16);
        std::vector<int> hit(tp, 0);
        for (int q = 0; q < tp; q++) {
            const int d = plane_piece(ne, q);
            REQUIRE(d >= 0 && d < tp);
            REQUIRE((q < 8 * ne) == (d < 8 * ne));
            if (q >= 8 * ne) REQUIRE(d == q);
            hit[d]++;
        }
        for (int q = 0; q < tp; q++) REQUIRE(hit[q] == 1);
    }

    // ---- every geometry the per-plane instantiation accepts ---------------------------------------------------------
    int n_geom = 0;
    size_t lds_max = 0;
    for (int ntaps = 16; ntaps <= 1536; ntaps++) {
        const Geom g = make_geom(ntaps, D, (unsigned)((ntaps - 1 + D - 1) / D * D), 0);
        if (!plane_form(D, g.ks, 0)) continue;
        n_geom++;
        const int ne = g.ne, e0 = g.e0, KP = g.ks / 2, TS = tile_stride(D, true);
        REQUIRE(ne == 152 && KP == 34);  // (what the kernel's constants assume)
        const size_t lds = lds_bytes(D, g.ks, ne, ntaps, true);
        REQUIRE(lds <= 160 * 1024);
        REQUIRE(lds > lds_bytes(D, g.ks, ne, ntaps, false));
        lds_max = lds > lds_max ? lds : lds_max;
        REQUIRE(!plane_form(D, g.ks, 8) && !plane_form(16, g.ks, 0));
        if (ntaps != 962 && ntaps != 1024 && ntaps != 1025) continue;  // (the layouts depend on ks, ne, e0 alone)

        // the table in global memory: piece ((f ne + E) 2 + part) 2 + pl holds digit plane 2 f + pl; staged
        const int tp = (int)((table_bytes(ne) + 15) / 16);
        std::vector<int> lds_tab(tp, -1);
        for (int q = 0; q < tp; q++) lds_tab[plane_piece(ne, q)] = q;
        for (int t = 0; t < KP; t++)
            for (int p = 0; p < 4; p++) {
                int addr[64], addr_old[64];
                for (int l = 0; l < 64; l++) {
                    const int r16 = l & 15, kq = l >> 4, i = r16 >> 1, part = r16 & 1;
                    const int off = plane_a_offset(ne, e0, p, t, r16, kq);
                    REQUIRE(off >= 0 && off % 16 == 0 && off / 16 < 8 * ne);
                    const int E = i - kq - 4 * t + e0;
                    REQUIRE(E >= 0 && E < ne);
                    REQUIRE(lds_tab[off / 16] == (((p >> 1) * ne + E) * 2 + part) * 2 + (p & 1));
                    addr[l] = off;
                    addr_old[l] = 16 * ((((p >> 1) * ne + E) * 2 + part) * 2 + (p & 1));  // T's own order
                    checked++;
                }
                REQUIRE(lds_cycles(addr) == 4);
                REQUIRE(lds_cycles(addr_old) == 8);
            }
        // the tile slot: 16 tiles a column block, the pair's 64 bytes of each
        const size_t slot = slot_bytes(D, g.ks, true);
        for (int t = 0; t < KP; t++)
            for (int j = 0; j < 4; j++) {
                int addr[64], addr_old[64];
                for (int l = 0; l < 64; l++) {
                    addr[l] = plane_b_offset(TS, j, t, l & 15, l >> 4);
                    REQUIRE(addr[l] + 16 <= (int)slot);
                    // (inside the tile's own 128 bytes: the padding is never read)
                    REQUIRE(addr[l] % TS + 16 <= tile_bytes(D));
                    addr_old[l] = plane_b_offset(tile_stride(D, false), j, t, l & 15, l >> 4);
                    checked++;
                }
                REQUIRE(lds_cycles(addr) == 4);
                REQUIRE(lds_cycles(addr_old) == 8);
            }
        // the landing's writes: lane l puts piece l + 64 u of the image at tile (l + 64 u) / 8, piece l % 8 -- eight
        // consecutive lanes, one of the store's lane groups, write one tile's 128 contiguous bytes: no conflict at any stride
        const int pieces = (int)(image_bytes(D, g.ks) / 16);
        for (int u = 0; 64 * u < pieces; u++) {
            int addr[64];
            for (int l = 0; l < 64; l++) {
                const int q = l + 64 * u;
                addr[l] = TS * (q / 8) + 16 * (q % 8);
                REQUIRE(addr[l] + 16 <= (int)slot);
            }
            REQUIRE(lds_write_cycles(addr) == 8);
        }
    }
    REQUIRE(n_geom == 1025 - 962 + 1);
    REQUIRE(lds_max == 161792);  // (1024 taps: two tables 39 424, counter 512, eight slots of 13 056, task scratch 17 408)

    // the strides beside 160 that the tile could take: 144 (the pair loop's), 176, 192, 208 conflict
    for (int ts : {144, 176, 192, 208}) {
        int addr[64];
        for (int l = 0; l < 64; l++) addr[l] = plane_b_offset(ts, 0, 0, l & 15, l >> 4);
        REQUIRE(lds_cycles(addr) == 8);
    }
    // (and the model on the plainest pattern: lane l at 16 l)
    {
        int addr[64];
        for (int l = 0; l < 64; l++) addr[l] = 16 * l;
        REQUIRE(lds_cycles(addr) == 4);
    }
    printf("plane_layout ok: %d geometries, %lld lane addresses checked, LDS at most %zu bytes\n", n_geom, checked, lds_max);
    return 0;
}
