"""tools/kernel_isa_digest.py: the per-kernel digest of a built object's machine code is a function of that kernel's code alone.
One object compared with itself reports no difference wherever it lies; the same source built with one -D changed reports exactly the
kernel whose body changed, with exit status 1; a kernel is matched to ITS code by mangled symbol even when a lambda the compiler keeps out
of line demangles to the same name in front of the argument list, and that lambda is a row of its own; the instruction count equals an
independent count of the kernel's lines in the disassembly."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from tests.conftest import REPO

sys.path.insert(0, os.path.join(REPO, 'tools'))

SMALL = 'heightmap.o'
HIPCC = '/opt/rocm/bin/hipcc'

# a kernel that calls a lambda kept out of line: the lambda demangles to `kern<2>(float*, int)::{lambda(float)#1}::operator()...`, whose
# text in front of the first '(' is the kernel's own name.  VARIANT changes the kernel's body only.
SOURCE = r'''
#include <hip/hip_runtime.h>
template <int K>
__global__ void kern(float* p, int n) {
  auto bump = [&](float x) __attribute__((noinline)) { return x * x + (float)K; };
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
#if VARIANT
  p[i] = bump(p[i]) + bump(p[i] + 1.0f) * 3.0f;
#else
  p[i] = bump(p[i]) + bump(p[i] + 1.0f);
#endif
}
template __global__ void kern<2>(float*, int);
__global__ void other(float* p) { p[threadIdx.x] += 1.0f; }
'''


@pytest.fixture(scope='module')
def two_copies(tmp_path_factory):
    import __graft_entry__ as g
    g.build()
    src = os.path.join(REPO, 'monoforce_amd', 'csrc', SMALL)
    a = tmp_path_factory.mktemp('digest_a')
    b = tmp_path_factory.mktemp('digest_b') / 'somewhere' / 'else'
    b.mkdir(parents=True)
    shutil.copy(src, a / SMALL)
    shutil.copy(src, b / SMALL)
    return str(a), str(b)


@pytest.fixture(scope='module')
def two_variants(tmp_path_factory):
    """The same source built twice, -DVARIANT=0 / 1, as `probe.o` in two directories."""
    root = tmp_path_factory.mktemp('digest_variants')
    (root / 'probe.hip').write_text(SOURCE)
    dirs = []
    for v in (0, 1):
        d = root / f'v{v}'
        d.mkdir()
        subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', f'-DVARIANT={v}', '-c', str(root / 'probe.hip'), '-o', str(d / 'probe.o')],
                       check=True, capture_output=True)
        dirs.append(str(d))
    return dirs


def test_object_compared_with_itself_reports_no_difference(two_copies, capsys):
    import kernel_isa_digest
    a, b = two_copies
    assert kernel_isa_digest.main([a, a]) == 0
    assert kernel_isa_digest.main([a, b, '--all']) == 0
    out = capsys.readouterr().out
    assert 'DIFFERS' not in out and 'ONLY IN' not in out and 'identical' in out, out


def test_digest_does_not_depend_on_the_path(two_copies):
    import kernel_isa_digest
    a, b = two_copies
    ta, tb = kernel_isa_digest.table(a), kernel_isa_digest.table(b)
    assert ta and ta == tb
    for (obj, sym), (name, count, sha, meta) in ta.items():
        assert obj == SMALL and count > 0 and len(sha) == 64, (name, count, sha, meta)
        assert meta is None or set(meta) == {'vgpr', 'agpr', 'sgpr', 'lds', 'scratch'}, (name, meta)


def test_changed_kernel_is_reported_and_only_that_kernel(two_variants, capsys):
    import kernel_isa_digest
    v0, v1 = two_variants
    assert kernel_isa_digest.main([v0, v1, '--all']) == 1
    out = capsys.readouterr().out
    rows = {re.sub(r'^\S+\s+(identical|DIFFERS)\s+\d+ ->\s+\d+\s+', '', ln): ln.split()[1] for ln in out.split('\n') if ' -> ' in ln}
    assert rows.get('kern<2>') == 'DIFFERS', out
    assert rows.get('other') == 'identical', out
    lam = [k for k in rows if k.startswith('(function)') and 'kern<2>' in k and 'lambda' in k]
    assert len(lam) == 1 and rows[lam[0]] == 'identical', out      # the out-of-line lambda: a row of its own, unchanged
    assert '1 differ' in out, out


def test_kernel_is_matched_to_its_own_code_and_counted_right(two_variants):
    """The kernel's row is the kernel's code, not the lambda's that shares its name up to the argument list; its instruction count is the
    number of instruction lines llvm-objdump prints between the kernel's symbol and the next one."""
    import kernel_isa_digest
    from kernel_metadata import LLVM
    v0, _ = two_variants
    t = kernel_isa_digest.table(v0)
    kern = [(sym, row) for (_, sym), row in t.items() if row[0] == 'kern<2>']
    lam = [(sym, row) for (_, sym), row in t.items() if row[0].startswith('(function)') and 'lambda' in row[0]]
    assert len(kern) == 1 and len(lam) == 1, sorted(r[0] for r in t.values())
    (ksym, (_, kcount, ksha, kmeta)), (lsym, (_, lcount, lsha, lmeta)) = kern[0], lam[0]
    assert kmeta is not None and lmeta is None and ksha != lsha and ksym != lsym
    co = os.path.join(v0, 'probe.co')
    assert kernel_isa_digest.code_object(os.path.join(v0, 'probe.o'), co)
    text = subprocess.run([f'{LLVM}/llvm-objdump', '-d', co], capture_output=True, text=True, check=True).stdout      # (with the raw bytes: another format)
    for sym, count in ((ksym, kcount), (lsym, lcount)):
        body = text.split(f'<{sym}>:\n', 1)[1].split('\n\n', 1)[0]
        lines = [ln for ln in body.split('\n') if ln.strip() and not re.match(r'^[0-9a-f]+ <', ln)]
        assert count == len(lines) and count > 0, (sym, count, len(lines))
    assert kcount != lcount
