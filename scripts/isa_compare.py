#!/usr/bin/env python3
"""Per-kernel comparison of two `hipcc -S` outputs (a refactor's gate: same code out of the compiler).

    hipcc <the build's flags> -x hip --cuda-device-only -S csrc/bn.hip -o parent/bn.s      (once per tree)
    isa_compare.py [--fold-encoding] [--pair PARENT=BRANCH ...] parent/bn.s branch/bn.s [more pairs ...]

One line per kernel: name, VGPRs, SGPRs, LDS bytes, scratch bytes, instruction count and "same", or what differs:
the .amdhsa resource lines (next_free_vgpr, next_free_sgpr, accum_offset, group_segment_fixed_size,
private_segment_fixed_size) and the multiset of instruction mnemonics, leaving out s_nop and s_waitcnt* (scheduling
artefacts).  Instruction order is not compared.  Exit status 1 when anything differs.
--pair PARENT=BRANCH (printed names) compares a parent kernel with a differently named branch kernel, which may serve several
parents; --fold-encoding counts v_x_e32 and v_x_e64 as v_x (the encoding the compiler picked, not the operation)."""
import collections
import re
import subprocess
import sys

RES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path, fold=False):
    s = open(path).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", s, re.M | re.S):
        name = m.group(1)
        res = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+)\s+(\d+)", m.group(2)) if k in RES}
        i = s.index("\n" + name + ":")
        j = s.index(".Lfunc_end", i)
        hist = collections.Counter()
        for line in s[i:j].split("\n")[1:]:
            t = line.split(";")[0].split()
            if not t or t[0].startswith(".") or t[0].endswith(":"):
                continue
            if t[0] == "s_nop" or t[0].startswith("s_waitcnt"):
                continue
            hist[re.sub(r"_e(32|64)$", "", t[0]) if fold else t[0]] += 1
        out[name] = (res, hist)
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt", "-p"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, (d.replace("void ", "").replace("mvg::", "") for d in r.stdout.split("\n"))))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    args = sys.argv[1:]
    fold = "--fold-encoding" in args
    pairs = [args[i + 1].split("=", 1) for i, x in enumerate(args[:-1]) if x == "--pair"]
    args = [x for i, x in enumerate(args) if x not in ("--fold-encoding", "--pair") and (i == 0 or args[i - 1] != "--pair")]
    if not args or len(args) % 2:
        sys.exit(__doc__)
    bad = 0
    for pa, pb in zip(args[0::2], args[1::2]):
        a, b = kernels(pa, fold), kernels(pb, fold)
        print(f"== {pa} -> {pb}: {len(a)} / {len(b)} kernels")
        pretty = demangle(sorted(set(a) | set(b)))
        renamed = {}                                             # parent's mangled name -> the paired branch kernel's
        for old, new in pairs:
            renamed.update({n: k for n in a for k in b if pretty[n] == old and pretty[k] == new})
        b = {**{k: v for k, v in b.items() if k not in renamed.values()}, **{n: b[k] for n, k in renamed.items()}}
        for n in sorted(set(a) ^ set(b)):
            print(f"  ONLY IN {'parent' if n in a else 'branch'}: {n}")
            bad += 1
        names = sorted(set(a) & set(b))
        for n in names:
            (ra, ha), (rb, hb) = a[n], b[n]
            diff = [f"{k} {ra.get(k)} -> {rb.get(k)}" for k in RES if ra.get(k) != rb.get(k)]
            diff += [f"{m} {ha[m]} -> {hb[m]}" for m in sorted(set(ha) | set(hb)) if ha[m] != hb[m]]
            bad += bool(diff)
            print(f"  {pretty[n]}{' = ' + pretty[renamed[n]] if n in renamed else ''}: vgpr {rb.get('next_free_vgpr')} sgpr {rb.get('next_free_sgpr')} lds {rb.get('group_segment_fixed_size')} "
                  f"scratch {rb.get('private_segment_fixed_size')} insts {sum(hb.values())}: {'same' if not diff else '; '.join(diff)}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
