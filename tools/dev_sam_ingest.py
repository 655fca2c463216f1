"""Kernel times of SAM text input: ms_lines, ms_encode and ms_keys of mgx_sam_stats over the synthetic record
set repeated to about 2.15 M records (text beyond the 256 MiB Infinity Cache), next to the inflate kernel's time on the same text.

    python tools/dev_sam_ingest.py [--records 2150000] [--runs 3]
"""
import argparse
import importlib
import os
import pathlib
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2_150_000)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    pkg = importlib.import_module("fast-genomic-data-processing_amd")
    import bam_cases as bm
    import sam_cases as sc
    syn = bm.synthetic(pkg.synth, pathlib.Path(tempfile.mkdtemp()))
    names, body = sc.sam_body(open(syn[0], "rb").read())
    reps = -(-a.records // len(syn[3]))
    text = np.frombuffer(body * reps, dtype=np.uint8)
    n_rec = len(syn[3]) * reps
    print(f"{len(text) / 2**20:.0f} MiB of text, {n_rec} lines, {len(text) / n_rec:.0f} bytes per line", flush=True)
    enc = pkg.SamEncoder(names)
    b = enc.batch(len(text), n_rec)
    rows = []
    for r in range(a.runs + 1):
        res = b.run(text, fetch=False)
        st = enc.stats()
        assert st["n_lines"] == n_rec and st["n_declined"] == 0 and len(res.keys) == n_rec
        if r:                                                     # the first run brings the code objects up
            rows.append((st["ms_lines"], st["ms_encode"], st["ms_keys"]))
    for k, name in enumerate(("lines", "size + encode", "keys")):
        v = [x[k] for x in rows]
        print(f"{name:14s} {min(v):8.3f} - {max(v):8.3f} ms ({len(text) / 1e6 / np.median(v):7.1f} GB/s of text)", flush=True)
    tot = [sum(x) for x in rows]
    print(f"{'all':14s} {min(tot):8.3f} - {max(tot):8.3f} ms ({len(text) / 1e6 / np.median(tot):7.1f} GB/s of text), {st['bytes_out'] / st['bytes_in']:.3f} bytes of BAM per byte of text", flush=True)
    b.close(); enc.close()
    # for scale, the same text back through the inflate kernel (BGZF made by the device compressor, blocks of 65280; the deflate
    # kernel's own rate on BAM bytes is in DESIGN.md 4.6: its stats cover the last batch of a call only, so it is not timed here)
    comp = pkg.BgzfCompressor(0)
    piece = 255 * 65280 * 16
    raw = np.concatenate([comp.compress(text[s:s + piece], block=65280)[0] for s in range(0, len(text), piece)])
    comp.close()
    off, isize, _, stop = pkg.bgzf.scan_blocks(raw)
    assert stop == 0 and int(isize.sum(dtype=np.uint64)) == len(text)
    inf = pkg.BgzfInflater(0)
    per, nb = 2048, len(isize)
    bt = inf.batch(per * 65536, per * 65536, per)
    for r in range(2):
        ms = 0.0
        for b0 in range(0, nb, per):
            cnt = min(per, nb - b0)
            lo, hi = int(off[b0]), int(off[b0 + cnt])
            bt.input[:hi - lo] = raw[lo:hi]
            bt.in_off[:cnt + 1] = off[b0:b0 + cnt + 1] - off[b0]
            bt.out_off[0] = 0
            bt.out_off[1:cnt + 1] = np.cumsum(isize[b0:b0 + cnt], dtype=np.uint64)
            bt.submit(cnt)
            _, _, err = bt.wait()
            assert err is None, err
            ms += inf.stats()["ms_kernel"]
    print(f"inflate kernel {ms:8.3f} ms ({len(text) / 1e6 / ms:7.1f} GB/s of text)", flush=True)
    bt.close(); inf.close()


if __name__ == "__main__":
    main()
