// window_reuse_layout.cpp -- the per-plane matrix loop that re-uses its tile windows (hz_firmm2.h, kReuse; the index maps
// are hz_firmm2_plan.h's reuse_row_offset, reuse_b_offset, reuse_b_reg, reuse_b_read and xchg_*) under AddressSanitizer +
// UndefinedBehaviorSanitizer.  Built by tests/test_window_reuse_layout.py:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I go-sdr_amd/csrc -I include
//         tests/host/window_reuse_layout.cpp -o window_reuse_layout
//   * the register rotation, simulated from the reads the loop issues (pair t + 1's in front of pair t's MFMAs, as the
//     loop has them): on every pair t, block j and lane (c, kq) the register the MFMA takes holds row 4 c + j + t / 2,
//     half t & 1, piece kq of the image -- and 40 B reads a pass do it;
//   * the LDS bank model of tests/host/plane_layout.cpp gives 4 cycles for every one of those reads, 8 with 16 bytes of
//     padding per four rows instead of 32, and more still with the kept loop's 160-byte rows: a model that could not tell
//     them apart would fail here;
//   * the landing's writes are conflict-free, rows do not overlap, and every row lies inside the image part of the slot;
//   * the LDS of every tap count the instantiation accepts fits a compute unit;
//   * the epilogue's exchange: in each of its two rounds no two writes meet, every byte read was written in that round, and
//     lane 32 h + n ends with y[b][a].part = output i = 4 h + a, part, of tile 32 b + n -- each of the 1024 values once;
//     its writes and reads are conflict-free by the same model.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
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

// ds_read_b128's lane groups (one LDS cycle each when conflict-free)
static const int kGroups[4][16] = {
    {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
    {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63},
};

// LDS-array cycles of one lane group: 16 bytes per lane at byte addresses addr[] (negative: the lane is switched off),
// `banks` banks of 4 bytes; equal addresses broadcast, N different addresses on a bank cost N cycles
static int group_cycles(const int (&addr)[64], const int *lanes, int n_lanes, int banks) {
    std::set<int> on_bank[64];
    for (int k = 0; k < n_lanes; k++) {
        const int a = addr[lanes[k]];
        if (a < 0) continue;
        REQUIRE(a % 16 == 0);
        for (int w = 0; w < 4; w++) on_bank[(a / 4 + w) % banks].insert(a / 4 + w);
    }
    size_t worst = 0;
    for (const auto &b : on_bank) worst = b.size() > worst ? b.size() : worst;
    return (int)worst;
}
static int lds_cycles(const int (&addr)[64]) {  // ds_read_b128
    int total = 0;
    for (const auto &grp : kGroups) total += group_cycles(addr, grp, 16, 64);
    return total;
}
static int lds_write_cycles(const int (&addr)[64]) {  // ds_write_b128: eight groups of eight consecutive lanes, 32 banks
    int total = 0;
    for (int g = 0; g < 8; g++) {
        int lanes[8];
        for (int k = 0; k < 8; k++) lanes[k] = 8 * g + k;
        total += group_cycles(addr, lanes, 8, 32);
    }
    return total;
}

struct Frag {  // what a B register of a lane holds
    int row, half, piece;
    bool operator==(const Frag &o) const { return row == o.row && half == o.half && piece == o.piece; }
};

int main() {
    constexpr int D = 8;
    static_assert(reuse_form(D, 68, kLoopReuse) && !reuse_form(D, 68, kLoopPlane) && !reuse_form(D, 68, kLoopPair), "the forms");
    static_assert(plane_form(D, 68, kLoopPlane) && plane_form(D, 68, kLoopReuse) && !reuse_form(16, 68, kLoopReuse), "the forms");
    static_assert(reuse_form(D, 68, 0) == (kLoopDefault == kLoopReuse), "the default is one of the two per-plane loops");
    long long checked = 0;

    int n_geom = 0;
    size_t lds_max = 0;
    for (int ntaps = 16; ntaps <= 1536; ntaps++) {
        const Geom g = make_geom(ntaps, D, (unsigned)((ntaps - 1 + D - 1) / D * D), 0);
        if (!reuse_form(D, g.ks, kLoopReuse)) continue;
        n_geom++;
        const int KP = g.ks / 2;
        REQUIRE(KP == 34);
        const size_t lds = form_lds_bytes(D, g.ks, g.ne, ntaps, true, true);
        REQUIRE(lds <= 160 * 1024);
        REQUIRE(lds <= lds_bytes(D, g.ks, g.ne, ntaps, true));  // (what the chain's eligibility check budgets)
        lds_max = lds > lds_max ? lds : lds_max;
        if (ntaps != 962 && ntaps != 1024 && ntaps != 1025) continue;  // (the layout depends on ks alone)

        const int rows = (int)(image_bytes(D, g.ks) / tile_bytes(D));
        const int image = (int)reuse_image_bytes(D, g.ks);
        REQUIRE(rows == 80);
        REQUIRE(reuse_slot_bytes(D, g.ks) == (size_t)image + kXchgBytes && image % 256 == 0);
        // rows: 128 contiguous bytes each, in order, apart, inside the image part of the slot
        std::map<int, int> row_of;  // byte offset of a 16-byte piece -> 8 row + piece
        for (int r = 0; r < rows; r++) {
            REQUIRE(reuse_row_offset(r) % 16 == 0 && reuse_row_offset(r) + 128 <= image);
            if (r) REQUIRE(reuse_row_offset(r) >= reuse_row_offset(r - 1) + 128);
            for (int p = 0; p < 8; p++) row_of[reuse_row_offset(r) + 16 * p] = 8 * r + p;
        }
        // (a lane's rows start at 4 c: ONE per-lane base, the rest constants)
        for (int c = 0; c < 16; c++)
            for (int r = 0; r < 20; r++) REQUIRE(reuse_row_offset(4 * c + r) == reuse_row_offset(4 * c) + reuse_row_offset(r));

        // ---- the rotation and the reads' cycles ---------------------------------------------------------------------
        std::vector<Frag> b(64 * 2 * 4, Frag{-1, -1, -1});  // b[lane][t & 1][register]
        int reads = 0, max_row = 0;
        auto load = [&](int t) {
            for (int j = 0; j < 4; j++) {
                if (!reuse_b_read(j, t)) continue;
                reads++;
                int addr[64], addr16[64], addr160[64];
                for (int l = 0; l < 64; l++) {
                    const int c = l & 15, kq = l >> 4;
                    addr[l] = reuse_b_offset(j, t, c, kq);
                    REQUIRE(row_of.count(addr[l]) == 1);
                    const int rp = row_of[addr[l]];
                    b[(l * 2 + (t & 1)) * 4 + reuse_b_reg(j, t)] = Frag{rp / 8, (rp % 8) / 4, rp % 4};
                    max_row = rp / 8 > max_row ? rp / 8 : max_row;
                    // the wrong layouts: 16 bytes per four rows; the kept loop's 160-byte rows
                    const int row = 4 * c + j + t / 2;
                    addr16[l] = 128 * row + 16 * (row >> 2) + 64 * (t & 1) + 16 * kq;
                    addr160[l] = tile_stride(D, true) * row + 64 * (t & 1) + 16 * kq;
                    checked++;
                }
                REQUIRE(lds_cycles(addr) == 4);
                REQUIRE(lds_cycles(addr16) == 8);
                REQUIRE(lds_cycles(addr160) > 8);
            }
        };
        load(0);
        for (int t = 0; t < KP; t++) {
            if (t + 1 < KP) load(t + 1);  // (in front of pair t's MFMAs: it must not touch what they take)
            for (int j = 0; j < 4; j++)
                for (int l = 0; l < 64; l++) {
                    const int c = l & 15, kq = l >> 4;
                    const Frag want{4 * c + j + t / 2, t & 1, kq};
                    REQUIRE(b[(l * 2 + (t & 1)) * 4 + reuse_b_reg(j, t)] == want);
                }
        }
        REQUIRE(reads == 8 + (KP - 2));  // 40 a pass
        REQUIRE(max_row == rows - 1);

        // ---- the landing: lane l puts piece l + 64 u at row (l + 64 u) / 8, piece l % 8 -- one address and constants ------
        const int pieces = (int)(image_bytes(D, g.ks) / 16);
        std::vector<int> hit(image / 16, 0);
        for (int u = 0; 64 * u < pieces; u++) {
            int addr[64];
            for (int l = 0; l < 64; l++) {
                const int q = l + 64 * u;
                addr[l] = reuse_row_offset(q / 8) + 16 * (q % 8);
                REQUIRE(addr[l] == reuse_row_offset(l / 8) + 16 * (l % 8) + u * reuse_row_offset(8));  // (the kernel's form)
                REQUIRE(addr[l] + 16 <= image);
                REQUIRE(row_of[addr[l]] == q);  // (piece q of the image is piece q % 8 of row q / 8)
                hit[addr[l] / 16]++;
            }
            REQUIRE(lds_write_cycles(addr) == 8);
        }
        for (int h : hit) REQUIRE(h <= 1);

        // ---- the exchange -----------------------------------------------------------------------------------------
        // value id: ((i 2 + part) 64 + T): output i, part of tile T
        std::vector<int> got(64 * 2 * 4 * 2, -1);  // [lane][b][a][part]
        for (int round = 0; round < 2; round++) {
            std::vector<int> mem(kXchgBytes / 4, -1);
            for (int j = 0; j < 4; j++) {
                int addr[64];
                for (int l = 0; l < 64; l++) {
                    addr[l] = -1;
                    if (xchg_half(l) != round) continue;
                    const int gq = l >> 4, c = l & 15;
                    addr[l] = xchg_write_offset(l, j);
                    REQUIRE(addr[l] >= 0 && addr[l] % 16 == 0 && addr[l] + 16 <= kXchgBytes);
                    REQUIRE(addr[l] == xchg_write_offset(l, j & 1) + 128 * (j >> 1));  // (the kernel's two addresses)
                    for (int k = 0; k < 4; k++) {
                        REQUIRE(mem[addr[l] / 4 + k] == -1);
                        mem[addr[l] / 4 + k] = ((2 * gq + (k >> 1)) * 2 + (k & 1)) * 64 + 4 * c + j;
                    }
                }
                // (four of the eight write groups are switched off: one cycle for each of the others)
                REQUIRE(lds_write_cycles(addr) == 4);
            }
            for (int q = 0; q < 2; q++) {
                int addr[64];
                for (int l = 0; l < 64; l++) {
                    addr[l] = xchg_read_offset(l, q);
                    REQUIRE(addr[l] >= 0 && addr[l] + 16 <= kXchgBytes);
                    for (int e = 0; e < 4; e++) {
                        const int v = mem[addr[l] / 4 + e];
                        REQUIRE(v >= 0);
                        got[((l * 2 + round) * 4 + 2 * q + (e >> 1)) * 2 + (e & 1)] = v;
                        checked++;
                    }
                }
                REQUIRE(lds_cycles(addr) == 4);
            }
        }
        std::set<int> seen;
        for (int l = 0; l < 64; l++)
            for (int bb = 0; bb < 2; bb++)
                for (int a = 0; a < 4; a++)
                    for (int part = 0; part < 2; part++) {
                        const int v = got[((l * 2 + bb) * 4 + a) * 2 + part];
                        const int h = l >> 5, n = l & 31;
                        REQUIRE(v == ((4 * h + a) * 2 + part) * 64 + 32 * bb + n);
                        seen.insert(v);
                    }
        REQUIRE(seen.size() == 1024);
    }
    REQUIRE(n_geom == 1025 - 962 + 1);
    REQUIRE(lds_max <= 163840);
    printf("window_reuse_layout ok: %d geometries, %lld lane addresses checked, LDS at most %zu bytes\n", n_geom, checked, lds_max);
    return 0;
}
