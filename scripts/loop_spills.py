#!/usr/bin/env python3
"""Where the SGPR-spill lane moves sit: for one kernel of snake_kernels.hip's
gfx950 assembly, every loop (a backward branch to an earlier label) with its
instruction count, v_writelane / v_readlane / scratch counts and the source
lines it spans (from -gline-tables-only .loc directives). VERDICT r2 item 2:
count the lane moves inside the draw-round and trace loops before changing them.

    python scripts/loop_spills.py [kernel-substring] [extra hipcc flags...]
    python scripts/loop_spills.py --sites k1 k2 ...   (one summary line per kernel)

--sites: every spill move (v_writelane into a spill VGPR, v_readlane from one)
with the source line it belongs to (the last .loc of a project file) and the
innermost loop around it (with that loop's source-line span): the moves on the
per-job path versus those inside the draw-round / trace / encode loops (VERDICT
r4 item 6).

Source lines are file:line of the files beside the source (csrc/: the kernels
and the step_*.h headers their device code is in); a span is one lo-hi range
per file, since a loop's instructions come from every function inlined into it.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.environ.get("SRC", os.path.join(ROOT, "marl-snake_amd", "csrc", "snake_kernels.hip"))
FLAGS = ['-O3', '-std=c++17', '-ffp-contract=off', '--offload-arch=gfx950', '-mllvm',
         '-amdgpu-atomic-optimizer-strategy=None', '--cuda-device-only', '-gline-tables-only']


def kernel_body(text, sub):
    for m in re.finditer(r'^(_Z\w+):[^\n]*$(.*?)^\.Lfunc_end', text, re.S | re.M):
        if sub in m.group(1):
            return m.group(1), m.group(2).splitlines()
    sys.exit('kernel not found: ' + sub)


def compile_asm(extra):
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, 'k.s')
        r = subprocess.run(['/opt/rocm/bin/hipcc'] + FLAGS + ['-S', SRC, '-o', asm] + extra,
                           capture_output=True, text=True)
        if r.returncode:
            sys.exit(r.stderr[-2000:])
        return open(asm).read()


def file_table(text):
    """.file number -> base name, for the files in the source's directory
    (.file N "dir" "name" or .file N "path"; relative to the compilation
    directory, which is file 0's or this process's)."""
    ents = {m.group(1): os.path.join(m.group(2), m.group(3)) if m.group(3) else m.group(2)
            for m in re.finditer(r'^\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', text, re.M)}
    m0 = re.search(r'^\s*\.file\s+0\s+"([^"]*)"\s+"', text, re.M)
    comp = m0.group(1) if m0 else os.getcwd()
    here = os.path.realpath(os.path.dirname(SRC))
    return {n: os.path.basename(p) for n, p in ents.items()
            if os.path.dirname(os.path.realpath(os.path.join(comp, p))) == here}


def instructions(text, lines):
    """The instruction stream as (text, (file, line) or None) and the label
    positions. The current line is the last .loc of a project file (line 0 is
    compiler-made code, other files are the HIP headers: both keep it)."""
    files = file_table(text)
    ins, labels, cur = [], {}, None
    for ln in lines:
        s = ln.strip()
        m = re.match(r'\.loc\s+(\d+)\s+(\d+)', s)
        if m:
            if m.group(1) in files and int(m.group(2)):
                cur = (files[m.group(1)], int(m.group(2)))
            continue
        m = re.match(r'^(\.LBB\w+):', s)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        if ln.startswith('\t') and s and not s.startswith(('.', ';')):
            ins.append((s, cur))
    loops = sorted({(labels[m.group(1)], j) for j, (s, _) in enumerate(ins)
                    for m in [re.match(r's_(?:cbranch_\w+|branch)\s+(\.LBB\w+)', s)]
                    if m and m.group(1) in labels and labels[m.group(1)] <= j})
    return ins, loops


def site(c):
    return '%s:%d' % c if c else '?'


def span(body):
    """One file:lo-hi per file of the instructions' source lines."""
    by = {}
    for _, c in body:
        if c:
            by.setdefault(c[0], []).append(c[1])
    return ['%s:%d-%d' % (f, min(v), max(v)) for f, v in sorted(by.items())]


def sites(text, sub):
    """Spill moves of one kernel by source line and innermost loop."""
    name, lines = kernel_body(text, sub)
    ins, loops = instructions(text, lines)
    spill_v = {m.group(1) for s, _ in ins for m in [re.match(r'v_writelane_b32\s+(v\d+)', s)] if m}
    by = {}
    for j, (s, line) in enumerate(ins):
        st = re.match(r'v_writelane_b32\s+(v\d+)', s)
        ld = re.match(r'v_readlane_b32\s+\w+,\s*(v\d+)', s)
        if not (st or (ld and ld.group(1) in spill_v)):
            continue
        inner = min((l for l in loops if l[0] <= j <= l[1]), key=lambda l: l[1] - l[0], default=None)
        if inner:
            key = f'loop {" ".join(span(ins[inner[0]:inner[1] + 1]))} ({inner[1] - inner[0] + 1} instructions)'
        else:
            key = 'straight-line'
        d = by.setdefault(key, {'stores': 0, 'reloads': 0, 'lines': set()})
        d['stores' if st else 'reloads'] += 1
        d['lines'].add(line)
    return {'kernel': name, 'instructions': len(ins), 'spill_vgprs': sorted(spill_v),
            'sites': {k: {'stores': v['stores'], 'reloads': v['reloads'],
                          'src_lines': [site(c) for c in sorted(v['lines'], key=lambda c: c or ('', 0))]}
                      for k, v in sorted(by.items())}}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--sites':
        text = compile_asm([])
        for sub in sys.argv[2:]:
            print(json.dumps(sites(text, sub)))
        return
    sub = sys.argv[1] if len(sys.argv) > 1 else 'k_autoresetILi4ELb0ELb0E'
    text = compile_asm(sys.argv[2:])
    name, lines = kernel_body(text, sub)
    ins, loops = instructions(text, lines)
    # spill VGPRs: the destinations of v_writelane (the code itself writes no
    # lanes); a v_readlane from one of them is a spill reload, the others are
    # the code's own broadcasts (readlane / twist neighbours)
    spill_v = {m.group(1) for s, _ in ins for m in [re.match(r'v_writelane_b32\s+(v\d+)', s)] if m}

    def reload(s):
        m = re.match(r'v_readlane_b32\s+\w+,\s*(v\d+)', s)
        return bool(m) and m.group(1) in spill_v
    out = []
    for a, b in loops:
        body = ins[a:b + 1]
        out.append({
            'first': a, 'last': b, 'instructions': len(body),
            'v_writelane': sum(s.startswith('v_writelane') for s, _ in body),
            'v_readlane': sum(s.startswith('v_readlane') for s, _ in body),
            'spill_reloads': sum(reload(s) for s, _ in body),
            'scratch_ops': sum(s.startswith(('scratch_', 'buffer_store', 'buffer_load')) for s, _ in body),
            'src_lines': span(body) or None,
        })
    print(json.dumps({'kernel': name, 'instructions': len(ins),
                      'v_writelane': sum(s.startswith('v_writelane') for s, _ in ins),
                      'v_readlane': sum(s.startswith('v_readlane') for s, _ in ins),
                      'spill_reloads': sum(reload(s) for s, _ in ins), 'spill_vgprs': sorted(spill_v)}))
    for o in out:
        print(json.dumps(o))


if __name__ == '__main__':
    main()
