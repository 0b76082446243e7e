#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, translation unit by translation unit.

    python tools/kernel_asm_diff.py OLD_TREE NEW_TREE [--jobs N] [--keep DIR] [--only a.hip,b.hip]

Every .hip file under chunkformer_amd/csrc of either tree is compiled for the device only
(`hipcc <build.py FLAGS + FILE_FLAGS> --cuda-device-only -S`) and the two assembly texts are compared
after dropping the lines that hold the per-compile `__hip_cuid_` symbol.

Per translation unit the tool prints "identical", or, where the texts differ, falls back to a
per-function comparison: every function of NEW_TREE must have the same body and the same
`.amdhsa_*` descriptor as its counterpart in OLD_TREE.  A counterpart is the function of the same symbol
name, or, for a kernel that lost or gained a template parameter, a function of the same base name whose
text is the same once its own symbol is replaced by a placeholder.  Functions that exist only in
OLD_TREE are listed as removed.  Exit status 1 if any function of NEW_TREE has no equal counterpart.

The comparison is on text and hashes only: it does not interpret instructions.

--keep DIR keeps the assembly as DIR/old/<tu>.s and DIR/new/<tu>.s; an existing DIR/old/<tu>.s is reused
(the old tree is taken to be an immutable checkout), DIR/new is always rebuilt.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("chunkformer_amd", "csrc")


def _build_cfg(tree):
    spec = importlib.util.spec_from_file_location("_cfm_build_cfg", os.path.join(tree, "chunkformer_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HIPCC, mod.FLAGS, mod.FILE_FLAGS


def _compile(tree, tu, out):
    hipcc, flags, file_flags = _build_cfg(tree)
    src = os.path.join(tree, CSRC, tu)
    cmd = [hipcc, *flags, *file_flags.get(tu, []), "--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src}:\n{r.stdout}\n{r.stderr}")
    return out


def _text(path):
    with open(path) as f:
        return [l for l in f.read().splitlines() if "__hip_cuid_" not in l]


# local labels carry the function's ordinal within the translation unit (.LBB4_7, .Lfunc_end4, and "BB4_7"
# in the compiler's loop comments): the ordinal shifts when another function is removed
_LOCAL = re.compile(r"(\.L|\b)(BB|func_end|func_begin|tmp)\d+")


def _functions(lines):
    """{symbol: normalised text of the function body + its kernel descriptor}."""
    body, desc = {}, {}
    i, n = 0, len(lines)
    while i < n:
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        if m:
            sym, j = m.group(1), i + 1
            while j < n and not re.match(r"\s*\.size\s+" + re.escape(sym) + ",", lines[j]):
                j += 1
            body[sym] = lines[i:j + 1]
            i = j + 1
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            sym, j = m.group(1), i + 1
            while j < n and ".end_amdhsa_kernel" not in lines[j]:
                j += 1
            desc[sym] = lines[i:j + 1]
            i = j + 1
            continue
        i += 1
    out = {}
    for sym, b in body.items():
        # the symbol also names the function's static __shared__ arrays (_ZZ<encoding>E...): drop the _Z
        core = sym[2:] if sym.startswith("_Z") else sym
        txt = "\n".join(b + ["--descriptor--"] + desc.get(sym, []))
        txt = _LOCAL.sub(lambda m: m.group(1) + m.group(2), txt.replace(core, "@SELF@"))
        txt = re.sub(r"[ \t]+", " ", txt)   # the comment column moves with a label's length
        out[sym] = hashlib.sha256(txt.encode()).hexdigest()
    return out


def _demangle(syms):
    if not syms:
        return {}
    filt = "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        r = subprocess.run([filt, *syms], capture_output=True, text=True, check=True)
        return dict(zip(syms, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {s: s for s in syms}


def _base(sym):
    """Qualified name without template arguments, from the mangled symbol's <length><identifier> prefix."""
    if not sym.startswith("_Z"):
        return sym
    rest, parts = sym[3:] if sym.startswith("_ZN") else sym[2:], []
    while rest and rest[0].isdigit():
        k = re.match(r"\d+", rest).group(0)
        parts.append(rest[len(k):len(k) + int(k)])
        rest = rest[len(k) + int(k):]
    return "::".join(parts)


def _compare_functions(old, new):
    fo, fn = _functions(old), _functions(new)
    names = _demangle(sorted(set(fo) | set(fn)))
    used, differ, mapped = set(), [], []
    for sym, h in fn.items():
        if sym in fo:
            used.add(sym)
            if fo[sym] != h:
                differ.append(names[sym])
            continue
        cands = [s for s in fo if s not in fn and _base(s) == _base(sym) and fo[s] == h]
        if cands:
            used.add(cands[0])
            mapped.append((names[cands[0]], names[sym]))
        else:
            differ.append(names[sym] + "   [no equal counterpart]")
    removed = [names[s] for s in fo if s not in used]
    return differ, mapped, removed


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--keep", default=None)
    ap.add_argument("--only", default=None, help="comma-separated translation units")
    a = ap.parse_args()

    tmp = None
    if a.keep:
        root = a.keep
    else:
        tmp = tempfile.TemporaryDirectory()
        root = tmp.name
    for side in ("old", "new"):
        os.makedirs(os.path.join(root, side), exist_ok=True)

    def tus(tree):
        return {f for f in os.listdir(os.path.join(tree, CSRC)) if f.endswith(".hip")}

    t_old, t_new = tus(a.old_tree), tus(a.new_tree)
    both = sorted(t_old | t_new)
    if a.only:
        both = [t for t in both if t in a.only.split(",")]

    jobs = []
    for tu in both:
        if tu in t_old:
            out = os.path.join(root, "old", tu + ".s")
            if not (a.keep and os.path.exists(out)):
                jobs.append((a.old_tree, tu, out))
        if tu in t_new:
            jobs.append((a.new_tree, tu, os.path.join(root, "new", tu + ".s")))
    # the weight-stationary GEMM units take minutes each: start them first
    jobs.sort(key=lambda j: 0 if "gemm_wst_" in j[1] else 1)
    with cf.ThreadPoolExecutor(max_workers=a.jobs) as ex:
        list(ex.map(lambda j: _compile(*j), jobs))

    bad = 0
    for tu in both:
        if tu not in t_old or tu not in t_new:
            print(f"{tu}: only in {'old' if tu in t_old else 'new'} tree")
            bad += tu in t_new
            continue
        old = _text(os.path.join(root, "old", tu + ".s"))
        new = _text(os.path.join(root, "new", tu + ".s"))
        if old == new:
            print(f"{tu}: identical")
            continue
        differ, mapped, removed = _compare_functions(old, new)
        if differ:
            bad += 1
            print(f"{tu}: DIFFERS in {len(differ)} function(s)")
            for d in differ:
                print(f"    differs: {d}")
        else:
            print(f"{tu}: every surviving function identical (text differs by removed/renamed functions)")
        for o, nn in mapped:
            print(f"    same code, renamed: {o}  ->  {nn}")
        for r in removed:
            print(f"    removed: {r}")
    if tmp:
        tmp.cleanup()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
