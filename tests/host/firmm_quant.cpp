// firmm_quant.cpp -- what the HIP-free planner headers (hz_firmm_plan.h, hz_firmm2_plan.h) make of a filter, printed
// for tests/firmm_ref.py: the exact reference of the int8 matrix FIR restates the quantisation in Python, and
// tests/test_firmm_ref_cpu.py holds that restatement against this program's output.  Built by firmm_ref.host_program:
//     g++ -std=c++17 -O1 -I go-sdr_amd/csrc tests/host/firmm_quant.cpp -o firmm_quant
//     firmm_quant <filters.bin> <tables: 0 | 1>
// filters.bin: records of three int32 (format: 0 i8, 1 u8; decimation D; ntaps) followed by ntaps complex64 taps.
// Per record, for a chain without a Shift stage (omega = 0, one table):
//     filter <index>
//     S <digit_shift>
//     combine_ok <int32_combine_ok>
//     geom_ok <the size conditions of the persistent passes: mm2_eligible's, from the header's own functions>
//     p0 <p0_lo> <p0_hi> <pairs = ks / 2>           (mm2 geometry + plane0_window)
//     geom <w0> <ks> <ne> <e0>                      (the geometry the tables below are built in)
//     dc <re> <im>                                  (hex floats)
//     q <re im re im ...>                           (digit_table's q_out)
//     tab1 <hex>  tab2 <hex>                        (tables = 1: the 4 * ne * 32 digit bytes, chunk and pass layout)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "hz_firmm_plan.h"

using namespace hz;

static bool geom_ok(int ntaps, int D) {
    if (!mm2::factor_ok((unsigned)D)) return false;
    const mm2::Geom g = mm2::make_geom(ntaps, D, 0, 0);
    return mm2::image_bytes(D, g.ks) <= (size_t)mm2::kU * 64 * 16 && mm2::table_bytes(g.ne) <= (size_t)4 * mm2::kThreads * 16 &&
           mm2::lds_bytes(D, g.ks, g.ne, g.ntaps, mm2::plane_form(D, g.ks, 0)) <= 160 * 1024 && g.ntaps + D * (mm2::kFixOut - 1) <= 5 * 256;
}

static void hex(const char *name, const uint8_t *p, size_t n) {
    printf("%s ", name);
    for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: firmm_quant <filters.bin> <tables: 0 | 1>\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    const bool tables = atoi(argv[2]) != 0;
    int32_t head[3];
    for (int index = 0; fread(head, sizeof head, 1, f) == 1; index++) {
        const bool u8 = head[0] != 0;
        const int D = head[1], nt = head[2];
        if (nt < 1 || nt > (1 << 20) || D < 1 || D % 8 != 0) {
            fprintf(stderr, "filter %d: bad header\n", index);
            return 2;
        }
        std::vector<float> t32(2 * (size_t)nt);
        if (fread(t32.data(), sizeof(float), t32.size(), f) != t32.size()) {
            fprintf(stderr, "filter %d: short read\n", index);
            return 2;
        }
        std::vector<double> taps(t32.begin(), t32.end());  // (the chain's taps_host: the float32 taps as doubles)
        const double scale = u8 ? 1.0 / 127.5 : 1.0 / 128.0;
        const int S = mm::digit_shift(taps.data(), (size_t)nt, scale);
        printf("filter %d\nS %d\n", index, S);
        printf("combine_ok %d\n", mm::int32_combine_ok(taps.data(), (size_t)nt, scale, S) ? 1 : 0);
        printf("geom_ok %d\n", geom_ok(nt, D) ? 1 : 0);
        const unsigned off = (unsigned)(nt - 1 + 7) / 8 * 8;
        const bool pass_geom = mm2::factor_ok((unsigned)D);
        mm::Geom g = mm::make_geom(nt, D, off, S);
        if (pass_geom) {
            mm2::Geom g2 = mm2::make_geom(nt, D, off, S);
            mm2::plane0_window(g2, D, taps.data(), scale);
            printf("p0 %d %d %d\n", g2.p0_lo, g2.p0_hi, g2.ks / 2);
            g.ntaps = g2.ntaps, g.w0 = g2.w0, g.ks = g2.ks, g.ne = g2.ne, g.e0 = g2.e0, g.shift = g2.shift, g.off = g2.off;
        } else {
            printf("p0 0 0 0\n");
        }
        printf("geom %d %d %d %d\n", g.w0, g.ks, g.ne, g.e0);
        std::vector<int64_t> q;
        const std::vector<uint8_t> tab1 = mm::digit_table(g, D, taps.data(), scale, 0.0, 0.0, u8, false, &q);
        double dc[2];
        memcpy(dc, tab1.data() + (size_t)4 * g.ne * 32, sizeof dc);
        printf("dc %a %a\n", dc[0], dc[1]);
        printf("q");
        for (size_t k = 0; k < q.size(); k++) printf(" %lld", (long long)q[k]);
        printf("\n");
        if (tables) {
            hex("tab1", tab1.data(), (size_t)4 * g.ne * 32);
            const std::vector<uint8_t> tab2 = mm::digit_table(g, D, taps.data(), scale, 0.0, 0.0, u8, true);
            hex("tab2", tab2.data(), (size_t)4 * g.ne * 32);
        }
    }
    fclose(f);
    return 0;
}
