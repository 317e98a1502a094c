"""The layer under the three decoder banks (csrc/hz_decodebank.h, csrc/hz_decodebank_plan.h) on the GPU: a Viterbi, an
LDPC and a Reed-Solomon bank are fed the SAME pattern of rows, slots and counts, and the set of slots each one writes is
compared with f < min(counts[r], cap) computed in numpy and with the other two.  The per-bank tests compare each bank
with its own reference program, which shares the bank's idea of a live slot; this is the property they cannot show.

The codes are the smallest at which each kernel still deals slots in groups: Viterbi K = 3, rate 1/2, 8 data bits, hard
input (16 frames per wave); the Hamming (7, 4) code, hard input (8 frames per workgroup); the Reed-Solomon code
(0x11D, 0, 1, 3, 4) at interleave 1 (1 frame per workgroup).  Every bank's data is one byte per frame.  The (rows, cap)
pairs put the slot totals at and one past 8 and 16 and a row boundary inside a group.  The counts cycle through 0, 1, cap
and cap + 5 row by row, from each of the four starting points (so that one row alone meets all four), and once there are
none; the destinations are dense, or views with pitches above the need; both memory spaces.  The frames are clean: a live slot
holds the planted byte and the info of a clean frame (Viterbi: metric 0 and, with no CRC configured, no verdict bit;
LDPC: 0 unsatisfied checks after 0 iterations, ok; Reed-Solomon: 0 errors, 0 failed, ok); every other byte, the pitch
padding included, and every other info word holds the fill."""
import importlib

import numpy as np
import pytest

import ldpc_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT8, SENT32 = 0xA5, 0xA5A5A5A5
RS_CODE = (0x11D, 0, 1, 3, 4)
VT_K, VT_GENS, VT_D = 3, (0o7, 0o5), 8
OK_INFO = {"viterbi": 0, "ldpc": 1 << 31, "rs": 1 << 31}
SHAPES = [(1, 1), (1, 17), (17, 1), (3, 3), (65, 2)]


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def contexts(hz):
    c = {"device": hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream), "host": hz.Context(0, hz.MEM_HOST)}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def hamming(hz):
    return hz.ldpc_systematic(hz.LdpcCode.from_dense(ldpc_ref.HAMMING74))[0]


def planted(hz, hamming, rows, cap, seed):
    """{bank: (frames (rows, cap, FB) uint8, the data byte of every slot (rows, cap) uint8)}: clean frames, none of 0xA5"""
    rng = np.random.default_rng(seed)

    def some_bytes():
        b = rng.integers(0, 255, (rows, cap)).astype(np.uint8)
        return np.where(b == SENT8, 0xFF, b).astype(np.uint8)
    vd, rd = some_bytes(), some_bytes()
    ld = (rng.integers(0, 16, (rows, cap)) << 4).astype(np.uint8)  # 4 data bits in front of a byte
    vf = np.zeros((rows, cap, 3), np.uint8)
    for r in range(rows):
        for f in range(cap):
            vf[r, f] = np.packbits(hz.conv_encode(np.unpackbits(vd[r, f:f + 1]), VT_K, VT_GENS))
    lf = np.packbits(hz.ldpc_encode(hamming, np.unpackbits(ld[..., None], axis=-1)[..., :4]), axis=-1)
    rf = hz.rs_encode(RS_CODE, rd[..., None])
    return {"viterbi": (vf, vd), "ldpc": (lf, ld), "rs": (rf, rd)}


@pytest.mark.parametrize("rows,cap", SHAPES)
@pytest.mark.parametrize("space", ["device", "host"])
def test_three_banks_write_the_same_slots(hz, contexts, hamming, space, rows, cap):
    ctx, device = contexts[space], space == "device"
    banks = {"viterbi": ctx.viterbi(hz.VITERBI_BITS, VT_K, VT_GENS, VT_D, rows=rows), "ldpc": ctx.ldpc(hz.LDPC_BITS, hamming, rows=rows),
             "rs": ctx.reed_solomon(RS_CODE, rows=rows)}
    assert banks["viterbi"].plan()[0] == 16 and banks["ldpc"].plan()[0] == 8 and banks["rs"].plan()[0] == 1
    assert [(b.frame_bytes, b.data_bytes) for b in banks.values()] == [(3, 1), (1, 1), (4, 1)]
    frames = planted(hz, hamming, rows, cap, 7 * rows + cap)

    def there(a):
        return torch.from_numpy(a).cuda() if device else a

    def back(a):
        return a.cpu().numpy() if device else a
    patterns = [np.array([(0, 1, cap, cap + 5)[(r + phase) % 4] for r in range(rows)], np.uint32) for phase in range(4)] + [None]
    for counts in patterns:
        live = np.arange(cap)[None, :] < (np.full(rows, cap) if counts is None else np.minimum(counts, cap))[:, None]
        cs = None if counts is None else there(counts.view(np.int32)) if device else counts
        for pitched in (False, True):
            written = {}
            for name, bank in banks.items():
                fr, want = frames[name]
                # dense, or slots and rows further apart than the data needs (the dense banks take a row pitch alone)
                shape = (rows, cap, 1) if not pitched else (rows, cap + 1, 4) if name == "rs" else (rows, cap + 2, 1)
                base = there(np.full(shape, SENT8, np.uint8))
                info = there(np.full((rows, cap), SENT32, np.uint32).view(np.int32 if device else np.uint32))
                bank.decode(there(fr), cs, cap, out=(base[:, :cap, :1], info))
                if device:
                    ctx.synchronize()
                got, words = back(base), back(info).view(np.uint32)
                expect = np.full(shape, SENT8, np.uint8)
                expect[:, :cap, 0][live] = want[live]
                assert np.array_equal(got, expect), (name, counts, pitched)
                assert np.array_equal(words, np.where(live, np.uint32(OK_INFO[name]), np.uint32(SENT32))), (name, counts, pitched)
                by_data, by_info = got[:, :cap, 0] != SENT8, words != SENT32
                assert np.array_equal(by_data, by_info), (name, counts, pitched)
                written[name] = by_info
            assert np.array_equal(written["viterbi"], live) and np.array_equal(written["ldpc"], live) and np.array_equal(written["rs"], live)
            assert np.array_equal(written["viterbi"], written["ldpc"]) and np.array_equal(written["ldpc"], written["rs"])
    for bank in banks.values():
        bank.close()
