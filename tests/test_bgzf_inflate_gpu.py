"""The device BGZF inflater (mgx_bgzf_inflate_*, mgx_bgzf_decompress): blocks made by zlib with every level, window,
memLevel and strategy over many kinds of data, blocks from the device compressor, htslib's own BAM files, a stream of
ragged blocks over several batches in flight, and corrupt blocks inside good batches -- the error names the block, the
other blocks are intact, the context stays usable."""
import gzip
import os

import numpy as np
import pytest

from conftest import ROOT
import bgzf_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inf(pkg):
    x = pkg.BgzfInflater(0)
    yield x
    x.close()


def run_batch(inf, blocks, isizes=None):
    isizes = isizes or [int.from_bytes(b[-4:], "little") for b in blocks]
    bt = inf.batch(max(1, sum(len(b) for b in blocks)), max(1, sum(isizes)), max(1, len(blocks)))
    try:
        n = bt.fill(blocks, isizes)
        bt.submit(n)
        return bt.wait()
    finally:
        bt.close()


def test_zlib_parameter_grid(inf):
    rng = np.random.RandomState(11)
    cases = bc.zlib_blocks(rng, n_random=3000)
    data, status, err = run_batch(inf, [b for b, _ in cases])
    assert err is None and not status.any(), err
    assert data == b"".join(w for _, w in cases)
    st = inf.stats()
    assert st["n_blocks"] >= len(cases) and st["bytes_out"] >= len(data) and st["ms_kernel"] > 0


def test_empty_one_byte_and_full_blocks_one_shot(inf):
    for d in (b"", b"x", bytes(range(256)) * 255):
        s = bc.bgzf(d, size=bc.MAX_IN)
        assert inf.decompress(s) == d
    assert inf.decompress(bc.EOF_BLOCK) == b""


def test_device_compressor_round_trip(pkg, inf, synth):
    data = synth.gen_bam_record_bytes(3_000_000, 5)
    comp = pkg.BgzfCompressor(0)
    blocks, _ = comp.compress(data)
    comp.close()
    assert inf.decompress(bytes(blocks) + bc.EOF_BLOCK) == data.tobytes()


def test_htslib_bam_files(inf):
    z = np.load(os.path.join(ROOT, "tests", "golden", "sam_vectors.npz"))
    for key in ("bin:range.bam", "bin:colons.bam"):
        raw = z[key].tobytes()
        assert inf.decompress(raw) == gzip.decompress(raw), key


def test_ragged_stream_over_batches_in_flight(pkg, inf):
    rng = np.random.RandomState(12)
    text = bc.sam_like(rng, 400_000)
    pool = [text, bytes(rng.randint(0, 256, 70000, dtype=np.uint8)), bytes(70000), bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 70000))]
    blocks, want = [], []
    for _ in range(12000):
        src = pool[int(rng.randint(len(pool)))]
        n = int(rng.choice([rng.randint(0, 100), rng.randint(0, 3000), rng.randint(0, bc.MAX_IN + 1)]))
        at = int(rng.randint(0, len(src) - n + 1))
        d = src[at:at + n]
        blocks.append(bc.block(d, level=int(rng.randint(0, 10)))); want.append(d)
    per = 1500
    batches = [inf.batch(per * 65536, per * 65536, per) for _ in range(3)]
    got = []
    try:
        flight = []
        for k, i in enumerate(range(0, len(blocks), per)):
            bt = batches[k % 3]
            if len(flight) == 3:
                data, status, err = flight.pop(0).wait()
                assert err is None, err
                got.append(data)
            bt.submit(bt.fill(blocks[i:i + per]))
            flight.append(bt)
        for bt in flight:
            data, status, err = bt.wait()
            assert err is None, err
            got.append(data)
    finally:
        for bt in batches:
            bt.close()
    assert b"".join(got) == b"".join(want)
    # and the one-shot path over the same stream (internal batches of 1024 blocks, two in flight)
    assert inf.decompress(b"".join(blocks)) == b"".join(want)


def test_corrupt_blocks_name_the_block_and_leave_the_context_usable(pkg, inf):
    rng = np.random.RandomState(13)
    text = bc.sam_like(rng, 300_000)
    good = [bc.block(text[i:i + 20000], level=6) for i in range(0, len(text), 20000)]
    crafted = dict(bc.crafted_bad_blocks())
    bad_crc = bytearray(good[4]); bad_crc[-8] ^= 1
    for name, bad, want_status in (("crc", bytes(bad_crc), 14), ("dist", crafted["dist_too_far"], 11),
                                   ("oversub", crafted["ll_oversubscribed"], 7), ("stored", crafted["stored_nlen"], 5)):
        blocks = list(good)
        pos = 4 if name == "crc" else 7
        blocks[pos] = bad
        data, status, err = run_batch(inf, blocks)
        assert err is not None and f"block {pos} " in err, (name, err)
        assert list(np.nonzero(status)[0]) == [pos] and status[pos] == want_status, (name, status)
        # the good blocks' bytes are in place
        offs = np.cumsum([0] + [int.from_bytes(b[-4:], "little") for b in blocks])
        for i, b in enumerate(blocks):
            if i != pos:
                assert data[offs[i]:offs[i + 1]] == text[i * 20000:(i + 1) * 20000]
    # a mutated stream: every corruption is an error or the right bytes, never a fault (the output ranges are the
    # original ISIZEs: a corrupted ISIZE is a mismatch the kernel reports)
    isizes = [int.from_bytes(b[-4:], "little") for b in good]
    offs = np.cumsum([0] + isizes)
    for k in range(200):
        blocks = [bc.mutate(rng, b) if rng.rand() < 0.3 else b for b in good]
        data, status, err = run_batch(inf, blocks, isizes)
        for i in range(len(blocks)):
            if status[i] == 0:
                assert data[offs[i]:offs[i + 1]] == text[i * 20000:(i + 1) * 20000], (k, i)
    # the context still works
    assert inf.decompress(b"".join(good)) == text
    # and the one-shot path names the bad block of the whole stream
    with pytest.raises(pkg.MgxError, match="block 9 "):
        inf.decompress(b"".join(good[:9] + [bytes(bad_crc)] + good[10:]))
