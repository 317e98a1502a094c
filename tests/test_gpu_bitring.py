"""The layer under the two bit-ring banks (csrc/hz_bitring.h, csrc/hz_framebank.h) on the GPU: a frame sync bank and an
HDLC bank take the SAME rows, push by push, and behind every push both banks' positions, last raw decisions and histories
are compared EXACTLY with plain numpy over the whole stream so far -- the sign bit, the differential decoding with
d[-1] = 0, the last K bits packed as the ABI says, zeros where the stream had not begun -- and with each other over the
bits both keep.  The per-bank tests compare each bank with its own reference program, which walks the same ring; fed a
ring broken for both banks alike they would still agree, and this is the property that would not.

The pushes are the smallest that cross a word (63, 64, 65), a chunk of 16 tiles (1023, 1024, 1025) and an empty push,
with ragged counts, in both memory spaces and under every differential decoding."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROWS, W, P, WORD, MAX_BYTES = 3, 8, 8, 0xB2, 4
K_FS, K_HD = W + P - 1, 8 * MAX_BYTES + 8 * MAX_BYTES // 5 + 8
PUSHES = (1, 63, 64, 65, 64 * 16 - 1, 64 * 16, 64 * 16 + 1, 0, 5)


@pytest.fixture(scope="module")
def hz():
    return importlib.import_module("go-sdr_amd")


@pytest.fixture(scope="module")
def contexts(hz):
    c = {"device": hz.Context(0, hz.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream), "host": hz.Context(0, hz.MEM_HOST)}
    yield c
    for x in c.values():
        x.close()


def history_of(raw, diff, K):
    """the raw decisions of a row so far -> the last K bits behind the decoding, packed: bit k in byte k / 8, bit 7 - k % 8"""
    prev = np.concatenate([[0], raw[:-1]]).astype(np.uint8)
    bits = raw if diff == 0 else (raw ^ prev if diff == 1 else 1 ^ raw ^ prev)
    return np.packbits(np.concatenate([np.zeros(K, np.uint8), bits.astype(np.uint8)])[-K:])


@pytest.mark.parametrize("diff", [0, 1, 2])
@pytest.mark.parametrize("space", ["device", "host"])
def test_both_banks_keep_the_same_stream(hz, contexts, space, diff):
    ctx, device = contexts[space], space == "device"
    rng = np.random.default_rng(100 + diff)
    fs = ctx.frame_sync(hz.SYMSYNC_REAL_F32, W, [WORD], [0], P, thr=0, diff=diff, rows=ROWS)
    hd = ctx.hdlc(hz.SYMSYNC_REAL_F32, diff=diff, max_bytes=MAX_BYTES, rows=ROWS)
    assert fs.history_bytes == (K_FS + 7) // 8 and hd.history_bytes == (K_HD + 7) // 8
    raw = [np.zeros(0, np.uint8) for _ in range(ROWS)]  # the raw decisions every row has consumed
    for n in PUSHES:
        x = rng.standard_normal((ROWS, n)).astype(np.float32)
        counts = np.array([n, rng.integers(0, n + 1), max(n - 1, 0)], np.uint32)
        for r in range(ROWS):
            raw[r] = np.concatenate([raw[r], (~np.signbit(x[r, :counts[r]])).astype(np.uint8)])
        xs, cs = (torch.from_numpy(x).cuda(), torch.from_numpy(counts.view(np.int32)).cuda()) if device else (x, counts)
        fs.push(xs, cs)
        hd.push(xs, cs)
        pf, _, yf, lf = fs.state()
        ph, _, _, yh, lh = hd.state()
        consumed = np.array([len(b) for b in raw], np.uint64)
        last = np.array([b[-1] if len(b) else 0 for b in raw], np.uint8)
        for got in (pf, ph, fs.positions(), hd.positions()):
            assert np.array_equal(got, consumed), (n, got, consumed)
        assert np.array_equal(lf, last) and np.array_equal(lh, last), (n, lf, lh, last)
        for r in range(ROWS):
            assert np.array_equal(yf[r], history_of(raw[r], diff, K_FS)), (n, r)
            assert np.array_equal(yh[r], history_of(raw[r], diff, K_HD)), (n, r)
            both = min(K_FS, K_HD)
            assert np.array_equal(np.unpackbits(yf[r])[:K_FS][-both:], np.unpackbits(yh[r])[:K_HD][-both:]), (n, r)
    fs.close()
    hd.close()
