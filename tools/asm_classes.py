"""Per-kernel compiler metadata and the LDS reads of the two-column loops, from the device assembly of mgx_pairhmm.hip
(hipcc -S --cuda-device-only with build.py's flags).  Prints, per pairhmm kernel: .vgpr_count, scratch bytes, and for
every self-loop block that reads two haplotype codes (the two-column loop of a cell form) its VALU count and LDS reads.
usage: asm_classes.py A.s [B.s]     (two files: side by side, in the format of profiles/*_ab.txt section 1)"""
import collections
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def short(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    return re.sub(r"\(.*$", "", name)


def parse(path):
    text = open(path).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n((?:\s+\.\w+:.*\n)+)", text):
        fields = dict(re.findall(r"\.(\w+):\s+(\S+)", m.group(2)))
        if "vgpr_count" in fields:
            meta[m.group(1)] = (int(fields["vgpr_count"]), int(fields.get("private_segment_fixed_size", 0)))
    loops = collections.defaultdict(list)
    for fm in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\s+s_endpgm", text, re.S | re.M):
        fn, body = fm.group(1), fm.group(2)
        blocks = re.split(r"^(\.LBB\d+_\d+):.*\n", body, flags=re.M)
        for label, blk in zip(blocks[1::2], blocks[2::2]):
            ins = [ln.split()[0] for ln in blk.split("\n") if ln.startswith("\t") and not ln.startswith("\t.") and not ln.startswith("\t;")]
            branch = re.findall(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", blk)
            if label not in branch or ins.count("ds_read_u8") != 2:
                continue
            lds = collections.Counter(i for i in ins if i.startswith("ds_") and i != "ds_read_u8")
            valu = sum(1 for i in ins if i.startswith("v_"))
            loops[fn].append(f"{valu} VALU, " + " + ".join(f"{n} {i}" for i, n in sorted(lds.items())))
    return meta, loops


def main():
    parsed = [parse(p) for p in sys.argv[1:3]]
    names = sorted({n for meta, _ in parsed for n in meta if "pairhmm_fwd" in n})
    dm = demangle(names)
    rows = sorted((short(dm[n]), n) for n in names)
    tags = ("parent", "new") if len(parsed) == 2 else ("",)
    for nice, n in rows:
        if "<double" in nice or "exact" in nice:
            continue
        cells = [f"{tag} vgpr/scratch {meta.get(n, ('-', '-'))}" for tag, (meta, _) in zip(tags, parsed)]
        print(f"{nice:44s} " + "  ".join(cells))
        for tag, (_, loops) in zip(tags, parsed):
            for k, desc in enumerate(loops.get(n, [])):
                print(f"    {tag} loop {k}: {desc}")


if __name__ == "__main__":
    main()
