"""Device BGZF inflate: kernel throughput on level-6 BGZF SAM text, and the sortmardup CLI on plain, BGZF and gzip input.

    python tools/dev_bgzf_inflate.py kernel [GB of text] [dir]
        SAM text from the synthetic generator, BGZF at zlib level 6 (host processes, 65 280-byte blocks); an A/B of 512,
        2048 and 8192 blocks per batch (kernel time); then batches of INFLATE_PER blocks (default 2048) inflated one at a
        time (kernel ms from HIP events, GB/s of inflated output, every batch checked against the text) and three in
        flight (pinned -> pinned, what the CLI sees).
    python tools/dev_bgzf_inflate.py cli [records] [dir]
        the CLI's wall clock on the same records as plain .sam, BGZF inflated on the device, BGZF with MGX_CLI_INFLATE=host
        (zlib on a gang of 16 threads per batch, beside the 16 parsers) and plain gzip (members of 64 MB each, zlib on the reader thread); outputs must be identical.
"""
import multiprocessing as mp
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import importlib  # noqa: E402

pkg = importlib.import_module("fast-genomic-data-processing_amd")
import bgzf_cases as bc  # noqa: E402

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E peak


def _bgzf_piece(args):
    path, a, b, level = args
    with open(path, "rb") as f:
        f.seek(a)
        d = f.read(b - a)
    return b"".join(bc.block(d[i:i + bc.MAX_IN], level=level) for i in range(0, len(d), bc.MAX_IN))


def _gzip_piece(args):
    path, a, b, level = args
    with open(path, "rb") as f:
        f.seek(a)
        d = f.read(b - a)
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(d) + c.flush()


def compress_file(src, dst, fn, piece, level=6):
    n = os.path.getsize(src)
    step = piece - piece % bc.MAX_IN
    jobs = [(src, a, min(n, a + step), level) for a in range(0, n, step)]
    with mp.Pool(16) as pool, open(dst, "wb") as out:
        for part in pool.imap(fn, jobs):
            out.write(part)
        if fn is _bgzf_piece:
            out.write(bc.EOF_BLOCK)
    return os.path.getsize(dst)


def make_sam(n_records, d):
    sam = os.path.join(d, f"inflate_{n_records}.sam")
    if not os.path.exists(sam):
        recs, _ = pkg.synth.gen_sortdedup_packed_fast(n_records, 0x5EED0007)
        pkg.synth.write_sam_from_packed(sam, recs)
    return sam


def kernel(gb, d):
    n_rec = int(gb * 1e9 / 360)
    t0 = time.time()
    sam = make_sam(n_rec, d)
    gzp = sam + ".bgzf6.gz"
    csize = compress_file(sam, gzp, _bgzf_piece, 64 * bc.MAX_IN)
    text_bytes = os.path.getsize(sam)
    print(f"{text_bytes / 1e9:.2f} GB of SAM text -> {csize / 1e9:.2f} GB of level-6 BGZF (ratio {text_bytes / csize:.2f}) in {time.time() - t0:.1f} s", flush=True)
    raw = np.fromfile(gzp, dtype=np.uint8)
    off, isize, _, stop = pkg.bgzf.scan_blocks(raw)
    assert stop == 0
    text = np.memmap(sam, dtype=np.uint8, mode="r")
    inf = pkg.BgzfInflater(0)
    nb = len(isize)
    # A/B: blocks per batch (one kernel runs at a time on the context's stream; a batch's blocks are the wavefronts it has)
    for per in (512, 2048, 8192):
        if per >= nb:
            break
        bt = inf.batch(per * 65536, per * 65536, per)
        ms = 0.0
        for first in range(0, nb - per + 1, per):
            cnt = min(per, nb - first)
            a, b = int(off[first]), int(off[first + cnt])
            bt.input[:b - a] = raw[a:b]
            bt.in_off[:cnt + 1] = off[first:first + cnt + 1] - off[first]
            bt.out_off[0] = 0
            bt.out_off[1:cnt + 1] = np.cumsum(isize[first:first + cnt], dtype=np.uint64)
            bt.submit(cnt)
            _, _, err = bt.wait()
            assert err is None
            ms += inf.stats()["ms_kernel"]
        n_out = int(isize[:(nb // per) * per].sum(dtype=np.uint64))
        print(f"  A/B {per:5d} blocks per batch: {n_out / ms / 1e6:.1f} GB/s of output (kernel time)", flush=True)
        bt.close()
    per = int(os.environ.get("INFLATE_PER", "2048"))
    batches = [inf.batch(per * 65536, per * 65536, per) for _ in range(3)]

    def fill(bt, first):
        cnt = min(per, nb - first)
        a, b = int(off[first]), int(off[first + cnt])
        bt.input[:b - a] = raw[a:b]
        bt.in_off[:cnt + 1] = off[first:first + cnt + 1] - off[first]
        bt.out_off[0] = 0
        bt.out_off[1:cnt + 1] = np.cumsum(isize[first:first + cnt], dtype=np.uint64)
        return cnt

    # 1. one batch at a time: kernel time alone
    ms_sum, out_sum, t_at = 0.0, 0, 0
    for first in range(0, nb, per):
        bt = batches[0]
        cnt = fill(bt, first)
        bt.submit(cnt)
        data, status, err = bt.wait()
        assert err is None, err
        assert data == text[t_at:t_at + len(data)].tobytes()
        t_at += len(data)
        ms_sum += inf.stats()["ms_kernel"]
        out_sum += len(data)
    print(f"kernel, batches of {per} blocks one at a time: {out_sum / 1e9:.2f} GB inflated in {ms_sum:.1f} ms of kernel time = "
          f"{out_sum / ms_sum / 1e6:.1f} GB/s of output ({100 * out_sum / ms_sum / 1e6 / HBM_PEAK_GBS:.2f} % of HBM peak; "
          f"{csize / ms_sum / 1e6:.1f} GB/s compressed in)", flush=True)
    # 2. three in flight, pinned in -> pinned out (verified on the first pass above)
    t0 = time.perf_counter()
    flight = []
    for k, first in enumerate(range(0, nb, per)):
        bt = batches[k % 3]
        if len(flight) == 3:
            _, _, err = flight.pop(0).wait()
            assert err is None
        bt.submit(fill(bt, first))
        flight.append(bt)
    for bt in flight:
        bt.wait()
    dt = time.perf_counter() - t0
    print(f"pipelined, three batches in flight (host fill of the pinned input included): {out_sum / dt / 1e9:.1f} GB/s of output", flush=True)
    for bt in batches:
        bt.close()
    inf.close()


def cli(n, d):
    import subprocess
    from test_cli_gpu import build_cli
    exe = build_cli()
    t0 = time.time()
    sam = make_sam(n, d)
    bg = sam + ".bgzf.gz"
    gz = sam + ".members.gz"
    compress_file(sam, bg, _bgzf_piece, 64 * bc.MAX_IN)
    compress_file(sam, gz, _gzip_piece, 64 << 20)
    print(f"{n} records: SAM {os.path.getsize(sam) / 1e9:.2f} GB, BGZF {os.path.getsize(bg) / 1e9:.2f} GB, gzip {os.path.getsize(gz) / 1e9:.2f} GB "
          f"({time.time() - t0:.0f} s to make)", flush=True)
    outs = {}
    for name, inp, env in (("plain .sam", sam, {}), ("BGZF, device inflate", bg, {}), ("BGZF, MGX_CLI_INFLATE=host", bg, {"MGX_CLI_INFLATE": "host"}),
                           ("plain gzip, host zlib", gz, {})):
        bam = os.path.join(d, "inflate_out.bam")
        t = time.perf_counter()
        res = subprocess.run([exe, "-I", inp, "-O", bam, "-t", "16"], capture_output=True, text=True, env=dict(os.environ, MGX_CLI_TRACE="1", **env))
        wall = time.perf_counter() - t
        assert res.returncode == 0, res.stderr[-2000:]
        ingest = [l for l in res.stdout.splitlines() if l.startswith("read + parse")]
        trace = [l.strip() for l in res.stderr.splitlines() if "inflate:" in l]
        print(f"{name:30s} wall {wall:6.2f} s   {ingest[0] if ingest else ''}   {trace[0] if trace else ''}", flush=True)
        with open(bam, "rb") as f:
            outs[name] = hash(f.read())
    assert len(set(outs.values())) == 1, "outputs differ"
    print("all four outputs identical", flush=True)
    for p in (sam, bg, gz):
        os.remove(p)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    d = sys.argv[3] if len(sys.argv) > 3 else "/dev/shm"
    if what == "kernel":
        kernel(float(sys.argv[2]) if len(sys.argv) > 2 else 2.0, d)
    else:
        cli(int(sys.argv[2]) if len(sys.argv) > 2 else 20_000_000, d)
