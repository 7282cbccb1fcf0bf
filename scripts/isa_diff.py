#!/usr/bin/env python3
"""Compare the gfx950 device assembly of the working tree with that of a git revision.

    python scripts/isa_diff.py <git-rev>

Every ``.hip`` unit of ``advanced_scrapper_amd/csrc`` is compiled device-only to assembly with the library's
build flags, once from an export of <git-rev> and once from the working tree.  The assembly is normalised
(comments from ``;`` to end of line, trailing blanks, empty lines, the source-hash ``__hip_cuid_`` symbol and
the function ordinal inside local labels are dropped) and compared function by function.  A refactor that claims "same code" shows every unit
identical; anything else lists the kernels that differ with their register, scratch and LDS figures before
and after and the head of a unified diff.  Exit status 1 if any unit differs.  Needs hipcc, no GPU.
"""
from __future__ import annotations

import difflib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join('advanced_scrapper_amd', 'csrc')
JOBS = 8            # compiles in flight (two trees x every unit); never sized by the machine
DIFF_LINES = 60     # "a screenful" of unified diff per kernel
# a block or function-end label carries its function's ordinal in the unit (.LBB7_3): a kernel that leaves or joins
# a unit renumbers every function after it, so the ordinal is dropped (the label stays unique inside its function)
LOCAL_LABEL = re.compile(r'(\.L(?:BB|func_begin|func_end|JTI))\d+')
FIGURES = ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size')


def _build_module():
    spec = importlib.util.spec_from_file_location('kw_build', os.path.join(ROOT, 'advanced_scrapper_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def export(rev: str, dest: str) -> None:
    """``git archive`` of <rev>'s csrc and include directories into dest."""
    ar = subprocess.Popen(['git', '-C', ROOT, 'archive', rev, CSRC, 'include'], stdout=subprocess.PIPE)
    subprocess.run(['tar', '-x', '-C', dest], stdin=ar.stdout, check=True)
    if ar.wait() != 0:
        sys.exit(f'isa_diff: cannot export {rev}')


def compile_unit(build, tree: str, unit: str, out: str) -> str:
    cmd = [build.HIPCC, f'--offload-arch={build.ARCH}', '-O3', '-std=c++17', '-fPIC',
           '--cuda-device-only', '-S', '-o', out, os.path.join(tree, CSRC, unit)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.exit(f'isa_diff: {" ".join(cmd)} failed:\n{r.stdout}')
    with open(out) as f:
        return f.read()


def normalise(asm: str) -> list[str]:
    out = []
    for line in asm.splitlines():
        line = line.split(';', 1)[0].rstrip()
        if line and '__hip_cuid_' not in line:
            out.append(LOCAL_LABEL.sub(r'\1', line))
    return out


def split_functions(lines: list[str]) -> dict[str, list[str]]:
    """{symbol: body} for every function (``.type sym,@function`` .. ``.size sym``); the rest of the
    file (kernel descriptors, metadata, data) goes under the key ''."""
    funcs: dict[str, list[str]] = {'': []}
    cur = ''
    for line in lines:
        m = re.match(r'\s*\.type\s+(\S+),@function', line)
        if m:
            cur = m.group(1)
            funcs[cur] = []
        funcs[cur].append(line)
        if cur and re.match(r'\s*\.size\s+' + re.escape(cur) + r'\b', line):
            cur = ''
    return funcs


def figures(lines: list[str], sym: str) -> dict[str, str]:
    """The kernel's entry of the ``amdhsa.kernels`` metadata; empty for a plain device function."""
    try:
        at = next(i for i, s in enumerate(lines) if re.match(r'\s+\.name:\s+' + re.escape(sym) + r'$', s))
    except StopIteration:
        return {}
    lo = at
    while not lines[lo].startswith('  - '):
        lo -= 1
    hi = at + 1
    while hi < len(lines) and lines[hi].startswith('   '):
        hi += 1
    out = {}
    for s in lines[lo:hi]:
        m = re.match(r'[\s-]+(\.\w+):\s+(\S+)$', s)
        if m and m.group(1) in FIGURES:
            out[m.group(1)] = m.group(2)
    return out


def compare(unit: str, old: list[str], new: list[str]) -> bool:
    if old == new:
        print(f'{unit}: identical ({len(new)} normalised lines)')
        return True
    fo, fn = split_functions(old), split_functions(new)
    names = [s for s in dict.fromkeys(list(fo) + list(fn)) if fo.get(s) != fn.get(s)]
    print(f'{unit}: DIFFERS in {", ".join(s or "(descriptors, metadata, data)" for s in names)}')
    for s in names:
        if not s:
            continue
        a, b = figures(old, s), figures(new, s)
        for k in FIGURES:
            if k in a or k in b:
                print(f'  {s} {k}: {a.get(k, "-")} -> {b.get(k, "-")}')
        diff = list(difflib.unified_diff(fo.get(s, []), fn.get(s, []), 'old', 'new', n=2, lineterm=''))
        for line in diff[:DIFF_LINES]:
            print('    ' + line)
        if len(diff) > DIFF_LINES:
            print(f'    ... {len(diff) - DIFF_LINES} more diff lines')
    return False


def main(argv: list[str]) -> int:
    if len(argv) != 2:
        sys.exit(__doc__)
    rev = argv[1]
    build = _build_module()
    units = sorted(f for f in os.listdir(os.path.join(ROOT, CSRC)) if f.endswith('.hip'))
    with tempfile.TemporaryDirectory(prefix='isa_diff_') as tmp:
        export(rev, tmp)
        old_units = sorted(f for f in os.listdir(os.path.join(tmp, CSRC)) if f.endswith('.hip'))
        with ThreadPoolExecutor(max_workers=JOBS) as pool:
            jobs = {(tag, u): pool.submit(compile_unit, build, tree, u, os.path.join(tmp, f'{tag}_{u}.s'))
                    for tag, tree, us in (('old', tmp, old_units), ('new', ROOT, units)) for u in us}
            asm = {k: normalise(j.result()) for k, j in jobs.items()}
    sha = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', rev], stdout=subprocess.PIPE, text=True).stdout.strip()
    print(f'device assembly, {build.ARCH}: {rev} ({sha}) against the working tree')
    same = True
    for u in sorted(set(units) | set(old_units)):
        if ('old', u) not in asm or ('new', u) not in asm:
            print(f'{u}: only in {"the working tree" if ("new", u) in asm else rev}')
            same = False
        else:
            same &= compare(u, asm[('old', u)], asm[('new', u)])
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main(sys.argv))
