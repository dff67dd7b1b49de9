#!/usr/bin/env python3
"""Static figures of every conv_ring_kernel instantiation in an assembly listing of csrc/conv_ring.hip:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -fno-slp-vectorize -Icsrc -Iinclude \
        csrc/conv_ring.hip -o ring.s          (a compile, not a run)
    python tools/ring_asm_stats.py ring.s

VGPR / SGPR / scratch / LDS bytes from the kernel descriptor; static counts of MFMA, ds_read_b128, ds_add_u32 and LDS-DMA
(global_load_lds_dwordx4) instructions; and the instructions per consumer step: the unrolled chunk body is the loop that
holds 180 MFMAs (9 steps x 20), its instruction count from the first to the last MFMA divided by 9.  Scratch accesses
inside that body are counted as well (a spill in the main loop)."""
import re
import sys


def kernels(text):
    """name -> list of instruction lines (labels, directives and comments dropped)."""
    out, name, body = {}, None, []
    for line in text.splitlines():
        m = re.match(r"^(_Z\w*conv_ring_kernel\w*):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        s = line.split(";")[0].strip()
        if s.startswith(".end_amdhsa_kernel") or s.startswith(".section"):
            out[name] = body
            name = None
            continue
        if not s or s.startswith(".") or s.endswith(":") or s.startswith("//"):
            continue
        body.append(s)
    return out


def meta(text):
    out = {}
    for m in re.finditer(r"\.group_segment_fixed_size: (\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size: (\d+)\s+"
                         r"\.sgpr_count:\s+(\d+).*?\.vgpr_count:\s+(\d+)", text, re.S):
        out[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), sgpr=int(m.group(4)), vgpr=int(m.group(5)))
    return out


def demangle(n):
    m = re.search(r"ILi(\d)ELb(\d)ELi(\d)ELb(\d)E(?:Li(\d)E)?", n)
    a = [int(v) for v in m.groups(default="1")]
    return "conv_ring_kernel<%d, %s, %d, %s, %d>" % (a[0], "true" if a[1] else "false", a[2], "true" if a[3] else "false", a[4])


def main():
    text = open(sys.argv[1]).read()
    md = meta(text)
    print("%-42s %5s %5s %7s %7s | %5s %8s %7s %8s | %s" % ("instantiation", "vgpr", "sgpr", "scratch", "lds", "mfma", "ds_rd128",
                                                           "ds_add", "lds_dma", "chunk body: instr / step, non-MFMA / step, scratch ops"))
    for name, body in kernels(text).items():
        cnt = lambda pat: sum(1 for s in body if re.match(pat, s))  # noqa: E731
        mf = [i for i, s in enumerate(body) if s.startswith("v_mfma")]
        # the consumer loop: the last run of 180 MFMAs (the epilogue has none)
        lo, hi = mf[-180], mf[-1]
        seg = body[lo:hi + 1]
        per = len(seg) / 9.0
        scr = sum(1 for s in seg if s.startswith("scratch_"))
        m = md.get(name, {})
        print("%-42s %5s %5s %7s %7s | %5d %8d %7d %8d | %.1f, %.1f, %d" % (
            demangle(name), m.get("vgpr"), m.get("sgpr"), m.get("scratch"), m.get("lds"), len(mf), cnt(r"ds_read_b128"),
            cnt(r"ds_add_u32"), cnt(r"global_load_lds_dwordx4"), per, per - 20.0, scr))


if __name__ == "__main__":
    main()
