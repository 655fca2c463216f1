"""The device BGZF inflater (mgx_bgzf_inflate_*, mgx_bgzf_decompress): blocks made by zlib with every level, window,
memLevel and strategy over many kinds of data, blocks from the device compressor, htslib's own BAM files, a stream of
ragged blocks over several batches in flight, hand-made members on the seams of the window expansion (token and byte
limits, sources across a window's start, link chains, stored blocks between Huffman blocks, ISIZE up to 65 536), and
corrupt blocks inside good batches -- the error names the block, the other blocks are intact, the context stays usable."""
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


# ---- the seams of the window expansion (bgzf_cases.window_seam_cases: hand-made members, zlib's inflate as the reference) ----
@pytest.fixture(scope="module")
def seams():
    return bc.window_seam_cases()


def check_batch(inf, cases):
    """one batch of (name, member, want): every status 0, every block's bytes equal to want"""
    data, status, err = run_batch(inf, [m for _, m, _ in cases])
    offs = np.cumsum([0] + [len(w) for _, _, w in cases])
    bad = [name for i, (name, _, w) in enumerate(cases) if status[i] != 0 or data[offs[i]:offs[i + 1]] != w]
    assert not bad and err is None and len(data) == offs[-1], (bad, err)


def test_window_seams_in_one_batch(inf, seams):
    check_batch(inf, seams)
    for case in seams:                                            # and each alone: a wavefront that has served no other block
        if case[0] in ("isize0", "isize65536", "win4353", "chain_dist1", "stored_only_empty"):
            check_batch(inf, [case])


def test_window_seams_between_ordinary_blocks_and_reversed(inf, seams):
    """One wavefront serves several blocks in turn (more blocks than the grid has wavefronts): the window, the token list
    and the tables in LDS must not leak from one block into the next, whatever the order."""
    rng = np.random.RandomState(14)
    text = bc.sam_like(rng, 60_000)
    plain = [("zlib%d" % i, bc.block(text[i * 3000:(i + 1) * 3000 + 17 * i], level=i % 10), text[i * 3000:(i + 1) * 3000 + 17 * i]) for i in range(len(seams))]
    mixed = [c for pair in zip(seams, plain) for c in pair]
    check_batch(inf, mixed)
    check_batch(inf, mixed[::-1])
    many = (mixed + mixed[::-1]) * 30                              # more blocks than 8 wavefronts on each of 256 CUs
    assert len(many) > 2 * 2048
    check_batch(inf, many)


def test_hostile_window_seams_inside_good_batches(pkg, inf, seams):
    hostile = bc.window_seam_hostile()
    assert sorted(s for _, _, s in hostile) == [11, 12, 14]
    good = [c for c in seams if c[0] in ("win4353", "src_mixed_periodic", "chain_dist1", "fixed_stored_fixed", "isize4097", "isize65536", "lit512")]
    assert len(good) == 7
    for name, bad, want_status in hostile:
        pos = 3
        blocks = [m for _, m, _ in good]
        blocks[pos] = bad
        data, status, err = run_batch(inf, blocks)
        assert err is not None and f"block {pos} " in err, (name, err)
        assert list(np.nonzero(status)[0]) == [pos] and status[pos] == want_status, (name, status)
        offs = np.cumsum([0] + [int.from_bytes(b[-4:], "little") for b in blocks])
        for i, (gname, _, w) in enumerate(good):
            if i != pos:
                assert data[offs[i]:offs[i + 1]] == w, (name, gname)
        check_batch(inf, good)                                     # the context is usable afterwards
    # every wavefront serves good and hostile blocks in turn: what a refused block leaves in LDS does not reach the next
    unit = [good[0], good[1], hostile[0], good[2], hostile[1], good[4], hostile[2]]
    blocks = [c[1] for c in unit] * 350
    assert len(blocks) > 2048
    data, status, err = run_batch(inf, blocks)
    assert list(status) == [0, 0, 11, 0, 12, 0, 14] * 350, err
    offs = np.cumsum([0] + [int.from_bytes(b[-4:], "little") for b in blocks])
    for i in range(len(blocks)):
        if status[i] == 0:
            assert data[offs[i]:offs[i + 1]] == unit[i % 7][2], (i, unit[i % 7][0])
    with pytest.raises(pkg.MgxError, match="block 2 "):
        inf.decompress(good[0][1] + good[1][1] + hostile[0][1] + good[2][1])
