#!/usr/bin/env python3
"""Compare the kernels of two device assembly files (hipcc ... --cuda-device-only -S).

    tools/isa_compare.py before.s after.s

One line per kernel symbol: register counts, scratch and LDS sizes, instruction count, and whether
the mnemonic histogram and the ordered skeleton (waits with operands, barriers, MFMAs, LDS-DMAs,
ds_read_b128, global loads and stores) are equal.  Kernels whose symbol changed (a dropped template
parameter) are paired in file order within the same function name.  Exit status 1 on any difference.
"""
import collections
import re
import sys

META = (".vgpr_count", ".sgpr_count", ".agpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
SKEL = re.compile(r"s_waitcnt|s_barrier|v_mfma|global_load|global_store|ds_read_b128")


def base_name(sym):
    m = re.search(r"\d([a-z]\w*?_kernel)", sym)
    return m.group(1) if m else sym


def parse(path):
    kernels, meta, cur, sym = collections.OrderedDict(), {}, None, None
    for line in open(path):
        m = re.match(r"^(\w+):", line)
        if m and cur is None:
            sym = m.group(1)
            cur = []
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                kernels[sym] = cur
                cur = None
                continue
            t = line.strip()
            if t and t[0] not in ".;" and not t.endswith(":"):
                t = t.split(";")[0].strip()
                cur.append(t)
        if re.match(r"  - \.\w+:", line):  # next kernel of amdhsa.kernels
            rec = {}
        m = re.match(r"  [- ] (\.\w+):\s+(\S+)", line)
        if m and m.group(1) in META:
            rec[m.group(1)] = m.group(2)
        elif m and m.group(1) == ".name":
            meta[m.group(2)] = rec
    return {k: (v, meta[k]) for k, v in kernels.items() if k in meta}


def describe(ins, md):
    hist = collections.Counter(i.split()[0] for i in ins)
    skel = [i if i.startswith("s_waitcnt") else i.split()[0] for i in ins if SKEL.match(i)]
    return dict(meta=tuple(md.get(k, "?") for k in META), n=len(ins), hist=hist, skel=skel)


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    pairs = [(k, k) for k in a if k in b]
    la = [k for k in a if k not in b]
    lb = [k for k in b if k not in a]
    bad = False
    for k in la:
        m = [j for j in lb if base_name(j) == base_name(k)]
        if m:
            pairs.append((k, m[0]))
            lb.remove(m[0])
        else:
            print(f"only before: {k}")
            bad = True
    for k in lb:
        print(f"only after:  {k}")
        bad = True
    print("# kernel | vgpr sgpr agpr scratch lds | instructions | histogram | skeleton")
    for ka, kb in pairs:
        da, db = describe(*a[ka]), describe(*b[kb])
        same_meta = da["meta"] == db["meta"]
        ok_h, ok_s = da["hist"] == db["hist"], da["skel"] == db["skel"]
        bad |= not (same_meta and ok_h and ok_s)
        name = ka if ka == kb else f"{ka} -> {kb}"
        fmt = lambda d: " ".join(d["meta"])
        print(f"{name} | {fmt(da)} -> {fmt(db) if not same_meta else 'same'} | {da['n']} -> {db['n']} | "
              f"{'equal' if ok_h else 'DIFFERENT'} | {'equal' if ok_s else 'DIFFERENT'} ({len(da['skel'])})")
        if not ok_h:
            d = {k: (da["hist"][k], db["hist"][k]) for k in set(da["hist"]) | set(db["hist"]) if da["hist"][k] != db["hist"][k]}
            print(f"    histogram: {d}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
