#!/usr/bin/env python3
"""Are the device functions of two source trees the same code?  Compiles the listed .hip files of either tree to gfx950
assembly with the flags of abacusutils_amd/csrc/Makefile plus `--cuda-device-only -S`, cuts the assembly into functions and
compares them by name across the trees.  Needs hipcc, no GPU.

    python scripts/kernel_isa_diff.py --a ../parent abacusutils_amd/csrc/pairs.hip \\
                                      --b . abacusutils_amd/csrc/{cellsort,pairs,pairs_jk,spheres,threepcf,fof}.hip

A function's text is its instructions, its basic-block labels with the function's number taken out (`.LBB12_3` -> `.LBB_3`:
the number counts the functions of a file), and the kernel descriptor (`.amdhsa_*`: registers, LDS, scratch); comment lines and
assembler bookkeeping are dropped.  Names are demangled and the namespaces of `--strip` (default: abacus::pairs, abacus and the
anonymous one) are taken out of them, so that code that moved between namespaces or files still meets its counterpart.  A name
that several files of a tree define (a kernel in a shared header) must be the same code in all of them.

Prints one line per function - `same` or `differ`, with the instruction counts of A and B - project functions first, then those
of the libraries (`rocprim::`, `hipcub::`), and ends with a summary.  Exit status 1 when a project function differs or is
missing on either side; library functions are reported only.  It reads text and looks for no particular instruction."""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

# abacusutils_amd/csrc/Makefile: CXXFLAGS, with CONTRACT apart
FLAGS = ['-O3', '-std=c++17', '-fPIC', '-munsafe-fp-atomics', '-Wall', '-Wno-unused-function']
FAST = ('fft.hip', 'xbin.hip', 'gfft.hip', 'shear.hip')       # the Makefile builds these with -ffp-contract=fast
LIBRARY = ('rocprim::', 'hipcub::')


def compile_to_asm(hipcc, arch, tree, rel, fast, out):
    src = (Path(tree) / rel).resolve()
    contract = '-ffp-contract=fast' if src.name in fast else '-ffp-contract=off'
    cmd = [hipcc, *FLAGS, f'--offload-arch={arch}', contract, '--cuda-device-only', '-S', str(src), '-o', str(out)]
    done = subprocess.run(cmd, cwd=src.parent, capture_output=True, text=True)
    if done.returncode:
        sys.exit(f'{" ".join(cmd)}\n{done.stderr}')
    return out.read_text()


def functions_of(asm):
    """{mangled name: [normalised lines]} of one assembly file"""
    found, name, body = {}, None, None
    descriptor = {}
    lines = asm.split('\n')
    for i, raw in enumerate(lines):
        line = raw.split(';', 1)[0].strip()
        if not line:
            continue
        m = re.match(r'\.type\s+(\S+),@function', line)
        if m:
            name, body = m.group(1), None
            continue
        if name and body is None and line == name + ':':
            body = []
            continue
        if body is not None:
            if line.startswith('.Lfunc_end'):
                found[name], name, body = body, None, None
            elif not line.startswith(('.Ltmp', '.p2align', '.cfi_', '.loc', '.file')):
                body.append(re.sub(r'\.LBB\d+_(\d+)', r'.LBB_\1', line))
            continue
        m = re.match(r'\.amdhsa_kernel\s+(\S+)', line)
        if m:
            end = next(j for j in range(i, len(lines)) if lines[j].strip() == '.end_amdhsa_kernel')
            descriptor[m.group(1)] = [re.sub(r'\s+', ' ', s.split(';', 1)[0].strip()) for s in lines[i + 1:end] if s.strip()]
    for kernel, block in descriptor.items():
        if kernel in found:
            found[kernel] = found[kernel] + block
    return found


def demangler(names):
    tool = next((t for t in ('/opt/rocm/lib/llvm/bin/llvm-cxxfilt', 'llvm-cxxfilt', 'c++filt')
                 if subprocess.run(['sh', '-c', f'command -v {t}'], capture_output=True).returncode == 0), None)
    names = sorted(names)
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input='\n'.join(names) + '\n', capture_output=True, text=True, check=True).stdout.split('\n')
    return dict(zip(names, out))


def load(hipcc, arch, tree, files, fast, strip, jobs, tmp, side):
    """{stripped demangled name: [(file, lines), ...]} of a tree"""
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        texts = list(pool.map(lambda k: compile_to_asm(hipcc, arch, tree, files[k], fast, Path(tmp) / f'{side}{k}.s'), range(len(files))))
    per_file = [functions_of(t) for t in texts]
    symbols = set()
    for funcs in per_file:
        symbols.update(funcs)
        for body in funcs.values():
            for line in body:
                symbols.update(re.findall(r'_Z[\w$.]+', line))
    plain = demangler(symbols)

    def clean(sym):
        text = plain.get(sym, sym)
        for ns in strip:
            text = text.replace(ns + '::', '')
        return text
    table = {}
    for rel, funcs in zip(files, per_file):
        for sym, body in funcs.items():
            body = [re.sub(r'_Z[\w$.]+', lambda m: clean(m.group(0)), line) for line in body]
            table.setdefault(clean(sym), []).append((rel, body))
    return table


def count(body):
    return sum(1 for line in body if not line.endswith(':') and not line.startswith('.'))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--a', nargs='+', required=True, metavar=('TREE', 'FILE'), help='a tree and its .hip files, relative to it')
    ap.add_argument('--b', nargs='+', required=True, metavar=('TREE', 'FILE'))
    ap.add_argument('--fast', nargs='*', default=list(FAST), metavar='NAME', help='file names built with -ffp-contract=fast')
    ap.add_argument('--strip', nargs='*', default=['abacus::pairs', 'abacus', '(anonymous namespace)'], metavar='NAMESPACE')
    ap.add_argument('--hipcc', default=os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'))
    ap.add_argument('--arch', default='gfx950')
    ap.add_argument('--jobs', type=int, default=8)
    ap.add_argument('--keep', metavar='DIR', default=None, help='keep the assembly files here')
    args = ap.parse_args()
    if len(args.a) < 2 or len(args.b) < 2:
        ap.error('--a and --b take a tree and at least one file')
    strip = sorted(args.strip, key=len, reverse=True)
    with tempfile.TemporaryDirectory() as scratch:
        tmp = args.keep or scratch
        Path(tmp).mkdir(parents=True, exist_ok=True)
        A = load(args.hipcc, args.arch, args.a[0], args.a[1:], args.fast, strip, args.jobs, tmp, 'a')
        B = load(args.hipcc, args.arch, args.b[0], args.b[1:], args.fast, strip, args.jobs, tmp, 'b')
    bad = 0
    for title, library in (('project', False), ('library', True)):
        names = sorted(n for n in set(A) | set(B) if any(tag in n for tag in LIBRARY) == library)
        tally = {'same': 0, 'differ': 0, 'missing': 0}
        print(f'== {title} functions')
        for n in names:
            if n not in A or n not in B:
                verdict, where = 'missing', f'only in {"B" if n not in A else "A"}: {", ".join(f for f, _ in (A.get(n) or B.get(n)))}'
            else:
                bodies = [body for _, body in A[n] + B[n]]
                verdict = 'same' if all(body == bodies[0] for body in bodies) else 'differ'
                where = f'{"/".join(str(count(b)) for _, b in A[n])} | {"/".join(str(count(b)) for _, b in B[n])}  ' \
                        f'{", ".join(f for f, _ in A[n])} | {", ".join(f for f, _ in B[n])}'
            tally[verdict] += 1
            print(f'{verdict:8s}{n}\n          {where}')
        print(f'== {title}: {len(names)} functions, {tally["same"]} same, {tally["differ"]} differ, {tally["missing"]} on one side only')
        if not library:
            bad = tally['differ'] + tally['missing']
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
