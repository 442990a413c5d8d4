#!/usr/bin/env python3
"""Per-kernel digests of the gfx950 device code, to prove a refactor neutral.

For every ``.hip`` under ``csrc/kernels`` the device side is compiled to
assembly with the flags ``build_native.py`` uses for that translation unit,
the text is cut per kernel symbol (instruction stream from the symbol's label
to its end label, plus its ``.amdhsa_kernel`` descriptor), comment lines and
``.file`` / ``.ident`` directives are dropped, and each piece is hashed.  The
assembly is treated as opaque text.

    python tools/kernel_digest.py -o new.json
    python tools/kernel_digest.py --root ../parent-checkout -o parent.json
    python tools/kernel_digest.py --compare parent.json new.json

``--compare`` prints every kernel that differs, is missing or is new and
exits 1 if there is one.
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
    """{kernel symbol: text of its instruction stream + descriptor block}."""
    lines = [l for l in asm.splitlines()
             if not l.lstrip().startswith(";") and not re.match(r"\s*\.(file|ident)\b", l)]
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
        while not re.match(r"\.Lfunc_end\d+:", lines[j]):
            j += 1
        pieces[name] = "\n".join(lines[i:j + 1] + d) + "\n"
    return pieces


def digest_tree(root, jobs):
    root = os.path.abspath(root)
    bn = load_build_native(root)
    kdir = os.path.join(root, PKG, "csrc", "kernels")
    srcs = sorted(os.path.join(kdir, f) for f in os.listdir(kdir) if f.endswith(".hip"))
    with tempfile.TemporaryDirectory() as tmp, \
            ThreadPoolExecutor(max_workers=min(MAX_JOBS, max(1, jobs))) as pool:
        asms = list(pool.map(lambda s: device_asm(bn, root, s, tmp), srcs))
    return {os.path.basename(s): {k: hashlib.sha256(t.encode()).hexdigest()
                                  for k, t in sorted(split_kernels(a).items())}
            for s, a in zip(srcs, asms)}


def compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    bad = 0
    for tu in sorted(set(a) | set(b)):
        ka, kb = a.get(tu, {}), b.get(tu, {})
        for k in sorted(set(ka) | set(kb)):
            if k not in kb:
                print(f"missing  {tu}  {k}")
            elif k not in ka:
                print(f"new      {tu}  {k}")
            elif ka[k] != kb[k]:
                print(f"differs  {tu}  {k}")
            else:
                continue
            bad += 1
    n = sum(len(v) for v in b.values())
    print(f"kernel_digest: {n} kernels in {b_path}, {bad} differing/missing/new against {a_path}")
    return 1 if bad else 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout to digest (default: the one this tool lives in)")
    ap.add_argument("-o", "--output", help="write the JSON here (default: stdout)")
    ap.add_argument("-j", "--jobs", type=int, default=MAX_JOBS, help=f"parallel compiles (at most {MAX_JOBS})")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    a = ap.parse_args(argv)
    if a.compare:
        return compare(*a.compare)
    text = json.dumps(digest_tree(a.root, a.jobs), indent=1, sort_keys=True) + "\n"
    if a.output:
        open(a.output, "w").write(text)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
