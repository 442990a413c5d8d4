#!/usr/bin/env python3
"""Per-kernel digests of the gfx950 device code, to prove a refactor neutral.

For every ``.hip`` under ``csrc/kernels`` the device side is compiled to
assembly with the flags ``build_native.py`` uses for that translation unit,
the text is cut per kernel symbol (instruction stream from the symbol's label
to its end label, plus its ``.amdhsa_kernel`` descriptor), comments,
``.file`` / ``.ident`` directives and the function numbers in local labels
are dropped, and each piece is hashed.  Beside
that hash the tool records a hash of the descriptor block alone (register
counts, accum offset, scratch, LDS: all that occupancy follows from) and the
number of instruction lines.  The assembly is treated as opaque text.

    python tools/kernel_digest.py -o new.json
    python tools/kernel_digest.py --root ../parent-checkout -o parent.json
    python tools/kernel_digest.py --compare parent.json new.json
    python tools/kernel_digest.py --compare parent.json new.json --by-symbol

``--compare`` prints every kernel that differs, is missing or is new and
exits 1 if there is one.  A differing kernel is reported as ``code differs,
descriptor same (Δ instructions ±n)`` or ``descriptor differs``.  With
``--by-symbol`` kernels are matched by symbol alone, so one that moved to
another translation unit unchanged is not reported, and a further unchanged
copy of a header's kernel is listed as ``copy`` and not counted.
"""
from __future__ import annotations

import argparse
import hashlib
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

MAX_JOBS = 16
PKG = "distributed_point_functions_amd"


def load_build_native(root):
    path = os.path.join(root, PKG, "build_native.py")
    spec = importlib.util.spec_from_file_location("_dpf_build_native", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def device_asm(bn, root, src, outdir):
    flags = [f for f in bn.HIP_FLAGS if f != "-shared"]
    if os.path.basename(src) in bn.DEFAULT_SCHED_TUS:
        flags = [f for f in flags if f not in bn.ILP_FLAGS]
    out = os.path.join(outdir, os.path.basename(src)[:-4] + ".s")
    cmd = [bn.HIPCC, *flags, f"-I{os.path.join(root, 'include')}", "--cuda-device-only", "-S",
           src, "-o", out]
    p = subprocess.run(cmd, cwd=root, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr)
        raise SystemExit(f"kernel_digest: {' '.join(cmd)} failed ({p.returncode})")
    return open(out).read()


def split_kernels(asm):
    """{kernel symbol: (text of its instruction stream, of its descriptor block)}."""
    lines = [l for l in asm.splitlines()
             if not l.lstrip().startswith(";") and not re.match(r"\s*\.(file|ident)\b", l)]
    # Local labels carry the function's number in its file (.LBB12_3,
    # .Lfunc_end12), and so do the comments behind them: both dropped, so a
    # kernel reads the same wherever it stands.
    lines = [re.sub(r"\.L(BB|JTI|CPI|func_begin|func_end)\d+", r".L\1", re.sub(r"\s*;.*$", "", l))
             for l in lines]
    desc, i = {}, 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = i
            while not re.match(r"\s*\.end_amdhsa_kernel\b", lines[j]):
                j += 1
            desc[m.group(1)] = lines[i:j + 1]
            i = j
        i += 1
    label = {}
    for n, l in enumerate(lines):
        m = re.match(r"(\S+):", l)
        if m and m.group(1) in desc:
            label[m.group(1)] = n
    pieces = {}
    for name, d in desc.items():
        if name not in label:
            raise SystemExit(f"kernel_digest: no label for kernel {name}")
        i = j = label[name]
        while not re.match(r"\.Lfunc_end:", lines[j]):
            j += 1
        pieces[name] = ("\n".join(lines[i:j + 1]) + "\n", "\n".join(d) + "\n")
    return pieces


def _sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def kernel_record(code, desc):
    """Labels and directives are not instructions; everything else indented is."""
    n = sum(1 for l in code.splitlines()
            if l[:1].isspace() and l.strip() and not l.lstrip().startswith("."))
    return {"sha256": _sha(code + desc), "descriptor": _sha(desc), "instructions": n}


def digest_tree(root, jobs):
    root = os.path.abspath(root)
    bn = load_build_native(root)
    kdir = os.path.join(root, PKG, "csrc", "kernels")
    srcs = sorted(os.path.join(kdir, f) for f in os.listdir(kdir) if f.endswith(".hip"))
    with tempfile.TemporaryDirectory() as tmp, \
            ThreadPoolExecutor(max_workers=min(MAX_JOBS, max(1, jobs))) as pool:
        asms = list(pool.map(lambda s: device_asm(bn, root, s, tmp), srcs))
    return {os.path.basename(s): {k: kernel_record(*t) for k, t in sorted(split_kernels(a).items())}
            for s, a in zip(srcs, asms)}


def _load(path):
    """{(tu, kernel): record}.  A bare hash (the earlier format) is a record
    with nothing but the hash."""
    out = {}
    for tu, ks in json.load(open(path)).items():
        for k, r in ks.items():
            out[tu, k] = dict(r, tu=tu) if isinstance(r, dict) else {"sha256": r, "tu": tu}
    return out


def _rekey_moved(a, b):
    """Kernels of b whose (tu, symbol) a lacks take the key of a kernel of a
    with the same symbol that b lacks (a header's kernel is in several files:
    the leftovers pair up in file order)."""
    only_a = sorted(k for k in a if k not in b)
    for key in sorted(k for k in b if k not in a):
        home = next((k for k in only_a if k[1] == key[1]), None)
        if home is not None:
            only_a.remove(home)
            b[home] = b.pop(key)
    # One more file carrying a header's kernel unchanged is no new kernel.
    known = {(k[1], r["sha256"]) for k, r in a.items()}
    for key in [k for k in b if k not in a and (k[1], b[k]["sha256"]) in known]:
        print(f"copy     {key[0]}  {key[1]}")
        del b[key]


def _how(ra, rb):
    if "descriptor" not in ra or "descriptor" not in rb:
        return "differs"
    if ra["descriptor"] != rb["descriptor"]:
        return "descriptor differs"
    return f"code differs, descriptor same (Δ instructions {rb['instructions'] - ra['instructions']:+d})"


def compare(a_path, b_path, by_symbol=False):
    a, b = _load(a_path), _load(b_path)
    if by_symbol:
        _rekey_moved(a, b)
    bad = 0
    for key in sorted(set(a) | set(b)):
        k = key[1]
        if key not in b:
            print(f"missing  {a[key]['tu']}  {k}")
        elif key not in a:
            print(f"new      {b[key]['tu']}  {k}")
        elif a[key]["sha256"] != b[key]["sha256"]:
            print(f"differs  {b[key]['tu']}  {k}: {_how(a[key], b[key])}")
        else:
            continue
        bad += 1
    n = len(b)
    print(f"kernel_digest: {n} kernels in {b_path}, {bad} differing/missing/new against {a_path}")
    return 1 if bad else 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout to digest (default: the one this tool lives in)")
    ap.add_argument("-o", "--output", help="write the JSON here (default: stdout)")
    ap.add_argument("-j", "--jobs", type=int, default=MAX_JOBS, help=f"parallel compiles (at most {MAX_JOBS})")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    ap.add_argument("--by-symbol", action="store_true",
                    help="with --compare: match kernels by symbol across translation units")
    a = ap.parse_args(argv)
    if a.compare:
        return compare(*a.compare, by_symbol=a.by_symbol)
    text = json.dumps(digest_tree(a.root, a.jobs), indent=1, sort_keys=True) + "\n"
    if a.output:
        open(a.output, "w").write(text)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
