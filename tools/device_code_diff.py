#!/usr/bin/env python3
"""Is the gfx950 code of two source trees the same?  For a host-only refactor it must be.

    python tools/device_code_diff.py OLD_TREE NEW_TREE [-j N] [--work DIR]

Compiles each translation unit of build_native.SOURCES in both flavours (shipped, -DPAVE_DIAG=1) with
build_native's flags plus --cuda-device-only, unbundles the gfx950 code object and compares .text as a
whole; where that differs (instantiation order moved), every FUNC symbol's name, size and code bytes
and every .kd descriptor.  Where a function's code differs the line says whether its descriptor (registers, LDS,
scratch) differs too.  Prints one line per file and flavour; exit status 1 on any difference."""
import argparse
import concurrent.futures
import hashlib
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pavenet_amd import build_native   # noqa: E402

LLVM = os.environ.get('ROCM_LLVM', '/opt/rocm/llvm/bin')
UNITS = [os.path.splitext(os.path.basename(src))[0] for src in build_native.SOURCES]
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'


def code_object(tree, unit, defs, tmp):
    src = os.path.join(tree, 'pavenet_amd', 'csrc', unit + '.hip')
    out = os.path.join(tmp, '%s%s_%s' % (unit, '_diag' if defs else '', hashlib.md5(tree.encode()).hexdigest()[:8]))
    deps = [os.path.join(d, f) for d in (os.path.dirname(src), os.path.join(tree, 'include')) for f in os.listdir(d)]
    if not (os.path.exists(out + '.o') and all(os.path.getmtime(out + '.o') >= os.path.getmtime(d) for d in deps)):
        subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-O3', '--offload-arch=gfx950',
                               '-std=c++17', '-fPIC', '-c', '--cuda-device-only'] + defs +
                              ['-I' + os.path.join(tree, 'include'), '-o', out + '.o', src])
    with open(out + '.o', 'rb') as f:
        bundled = f.read(24) == b'__CLANG_OFFLOAD_BUNDLE__'
    if not bundled:
        return out + '.o'
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o', '--unbundle',
                           '--targets=' + TARGET, '--input=' + out + '.o', '--output=' + out + '.co'])
    return out + '.co'


def symbols(path):
    """.text hash, and {symbol: (size, bytes)} for the functions and the kernel descriptors."""
    blob = open(path, 'rb').read()
    secs = {}   # index -> (name, addr, offset, size)
    for line in subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '-S', '-W', path], text=True).splitlines():
        f = line.replace('[', ' ').replace(']', ' ').split()
        if len(f) >= 6 and f[0].isdigit() and f[2] in ('PROGBITS', 'NOBITS'):
            secs[int(f[0])] = (f[1], int(f[3], 16), int(f[4], 16), int(f[5], 16))
    text = next(s for s in secs.values() if s[0] == '.text')
    syms = {}
    for line in subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '-s', '-W', path], text=True).splitlines():
        f = line.split()
        if len(f) == 8 and f[0].endswith(':') and f[6].isdigit() and (f[3] == 'FUNC' or f[7].endswith('.kd')):
            _, addr, off, _ = secs[int(f[6])]
            start = int(f[1], 16) - addr + off
            code = blob[start:start + int(f[2])]
            if f[7].endswith('.kd'):   # bytes 16 .. 23: the entry's offset from the descriptor, moves with the order
                code = code[:16] + code[24:]
            syms[f[7]] = (int(f[2]), code)
    return hashlib.sha256(blob[text[2]:text[2] + text[3]]).hexdigest(), syms


def compare(old, new, unit, defs, tmp):
    (ht_a, a), (ht_b, b) = (symbols(code_object(t, unit, defs, tmp)) for t in (old, new))
    label = '%-20s %-8s' % (unit + '.hip', 'diag' if defs else 'shipped')
    kernels = sum(1 for s in a if s.endswith('.kd'))
    if ht_a == ht_b and a == b:
        return True, '%s identical: .text sha256 %s, %d kernels, %d symbols' % (label, ht_a[:16], kernels, len(a))
    bad = sorted(s for s in set(a) | set(b) if a.get(s) != b.get(s))
    if not bad:
        return True, '%s identical per symbol (order moved): %d kernels, %d symbols' % (label, kernels, len(a))
    notes = []
    for s in bad:
        if not s.endswith('.kd'):
            kd = 'absent' if s + '.kd' not in a else 'differs' if s + '.kd' in bad else 'identical'
            notes.append('%s (%s -> %s bytes, .kd %s)' % (s, a[s][0] if s in a else '-', b[s][0] if s in b else '-', kd))
        elif s[:-3] not in bad:
            notes.append(s + ' (code identical)')
    return False, '%s DIFFERS in %d of %d symbols: %s' % (label, len(bad), len(set(a) | set(b)), ', '.join(notes))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('-j', type=int, default=4)
    ap.add_argument('--work', help='keep the code objects here and reuse those newer than their sources')
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as scratch, concurrent.futures.ThreadPoolExecutor(args.j) as pool:
        tmp = args.work or scratch
        os.makedirs(tmp, exist_ok=True)
        jobs = [pool.submit(compare, os.path.abspath(args.old), os.path.abspath(args.new), u, d, tmp)
                for u in UNITS for d in ([], ['-DPAVE_DIAG=1'])]
        results = [j.result() for j in jobs]
    print('\n'.join(msg for _, msg in results))
    return 0 if all(ok for ok, _ in results) else 1


if __name__ == '__main__':
    sys.exit(main())
