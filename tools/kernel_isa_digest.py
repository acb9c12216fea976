"""Per-kernel digest of the machine code in the built translation units: did a change of the source change a kernel?

    python tools/kernel_isa_digest.py <csrc dir A> [<csrc dir B>] [--units a,b,...] [--all]

For every kernel of every `*.o` under a directory (or of the objects named by --units, without the suffix), matched by mangled
symbol, and for every other function the code object keeps out of line (rows of their own): the number of
instructions and a sha256 over the disassembly (`llvm-objdump -d --no-show-raw-insn` of the gfx950 code object, unbundled as
tools/kernel_metadata.py does; addresses, comments and blank lines dropped, so a kernel that only moved inside its object hashes
the same).  With two directories: the rows whose digest or metadata row (vgpr / agpr / sgpr / lds / scratch) differs, and the
rows present on one side only; --all prints every row with its verdict.  Exit status 1 when anything differs.

It hashes whole kernels; which instruction changed is a question for a `hipcc -S` listing and tools/loop_stats.py."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_metadata import LLVM, kernels  # noqa: E402

_SYM = re.compile(r'^[0-9a-f]+ <(\S+)>:\s*$')
_ADDR = re.compile(r'^\s*[0-9a-f]+:\s*')


def code_object(obj, out):
    """Unbundle the gfx950 code object of `obj` into the file `out`; False for a host-only object."""
    fb = out + '.fb'
    if subprocess.run([f'{LLVM}/llvm-objcopy', '--dump-section', f'.hip_fatbin={fb}', obj], capture_output=True).returncode:
        return False
    subprocess.run([f'{LLVM}/clang-offload-bundler', '--unbundle', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950',
                    f'--input={fb}', f'--output={out}'], capture_output=True, text=True, check=True)
    return True


def digests(obj):
    """{mangled symbol: (instruction count, sha256 hex)} over the functions of one object's code object."""
    with tempfile.TemporaryDirectory() as td:
        co = os.path.join(td, 'co')
        if not code_object(obj, co):
            return {}
        text = subprocess.run([f'{LLVM}/llvm-objdump', '-d', '--no-show-raw-insn', co], capture_output=True, text=True, check=True).stdout
    out, name, count, h = {}, None, 0, None
    for line in text.split('\n'):
        m = _SYM.match(line)
        if m:
            if name is not None:
                out[name] = (count, h.hexdigest())
            name, count, h = m.group(1), 0, hashlib.sha256()
            continue
        if name is None:
            continue
        line = _ADDR.sub('', line.split('//')[0]).strip()
        if line:
            count += 1
            h.update(line.encode() + b'\n')
    if name is not None:
        out[name] = (count, h.hexdigest())
    return out


def table(csrc, units=None):
    """{(object, symbol): (name, instructions, sha256, metadata dict or None)} over the functions of a built csrc directory.  Kernels
    are matched to their code by MANGLED symbol and carry their metadata row.  Every other function of a code object -- a device
    function or lambda the compiler left out of line -- is a row of its own (full demangled signature, metadata None): a kernel that
    calls it changes when either row does."""
    meta = kernels(csrc, mangled=True)
    objs = sorted({o for o, _, _, _ in meta})
    if units is not None:
        objs = [o for o in objs if o[:-2] in units]
    rows = {}
    for o in objs:
        d = digests(os.path.join(csrc, o))
        kern = {sym: (n, m) for oo, n, m, sym in meta if oo == o}
        missing = sorted(set(kern) - set(d))
        if missing:
            raise RuntimeError(f'{o}: no code found for the kernels {missing}')
        others = sorted(set(d) - set(kern))
        full = subprocess.run(['c++filt'], input='\n'.join(others), capture_output=True, text=True).stdout.split('\n')
        for sym, (n, m) in kern.items():
            rows[(o, sym)] = (n,) + d[sym] + (m,)
        for sym, n in zip(others, full):
            rows[(o, sym)] = ('(function) ' + n,) + d[sym] + (None,)
    return rows


def _meta(m):
    return ' '.join(f'{k} {m[k]}' for k in ('vgpr', 'agpr', 'sgpr', 'lds', 'scratch')) if m else '(not a kernel)'


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('a')
    ap.add_argument('b', nargs='?')
    ap.add_argument('--units', help='comma-separated object names without .o (default: every object)')
    ap.add_argument('--all', action='store_true', help='with two directories: print the identical rows too')
    args = ap.parse_args(argv)
    units = set(args.units.split(',')) if args.units else None
    ta = table(args.a, units)
    order = lambda t: sorted(t, key=lambda k: (k[0], t[k][0], k[1]))  # noqa: E731
    if args.b is None:
        for o, sym in order(ta):
            n, cnt, h, m = ta[(o, sym)]
            print(f'{o:36s} {cnt:6d} {h[:16]}  {_meta(m)}  {n}')
        return 0
    tb = table(args.b, units)
    differ = 0
    both = {**tb, **ta}
    for key in order(both):
        o, n = key[0], both[key][0]
        if key not in ta or key not in tb:
            differ += 1
            print(f'{o:36s} ONLY IN {"A" if key in ta else "B"}  {n}')
            continue
        (_, ca, ha, ma), (_, cb, hb, mb) = ta[key], tb[key]
        same = ha == hb and ma == mb
        differ += not same
        if same and not args.all:
            continue
        print(f'{o:36s} {"identical" if same else "DIFFERS  "} {ca:6d} -> {cb:6d}  {n}')
        if ma != mb:
            print(f'{"":36s}   A: {_meta(ma)}\n{"":36s}   B: {_meta(mb)}')
    print(f'{len(set(ta) & set(tb))} functions on both sides, {differ} differ')
    return 1 if differ else 0


if __name__ == '__main__':
    sys.exit(main())
