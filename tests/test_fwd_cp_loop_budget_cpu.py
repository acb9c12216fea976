"""Issue-slot budget of the component-parallel forward's step loops (rollout_fwd_cp_kernel.h).  These kernels run one wave per SIMD: a wave
alone issues one instruction per ~4 cycles whatever it is, so the instruction count of the step loop IS the kernel's time.  The listing
of rollout_fwd_cp_fast.hip, compiled with the Makefile's own command line, is held to
  * at most 270 instructions per trip (two steps, the closing branch included) in the loop of the fit step's forward (default
    integrator, separate maps, record, no forces, no fused loss) -- 287 before the loop took its cross-lane operands inside the
    arithmetic instructions, dropped the clamps of its prefetch offsets and chose its friction form in front of the loop;
  * no more than the count of the commit before that in every other instantiation, dynamics() included (PARENT below);
  * the distance the compiler cannot check: a DPP instruction written as inline assembly reads its DPP operand no sooner than two wait
    states after the instruction that wrote it.
Every kernel holds its step loop twice (with and without a friction map: the wave picks one in front of the loop); both are held."""
import os
import re
import shutil
import subprocess

import pytest

from tests.conftest import REPO

CSRC = os.path.join(REPO, 'monoforce_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc'
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which('make') is None, reason='needs hipcc and make')

FIT_STEP_FORWARD = (1, 0, 0, 1, 0)
BUDGET = 270
# (INTEG, FORCES, ZMU, REC, LOSS) -> instructions of the step loop, closing branch included, at the parent commit (fb74be7): per two
# steps for the default integrator (INTEG = 1), per step for dynamics()
PARENT = {
    (1, 0, 1, 1, 1): 321, (1, 0, 0, 1, 1): 324, (1, 0, 1, 0, 1): 314, (1, 0, 0, 0, 1): 319,
    (1, 1, 1, 1, 0): 294, (1, 1, 1, 0, 0): 291, (1, 1, 0, 1, 0): 296, (1, 1, 0, 0, 0): 291,
    (1, 0, 1, 1, 0): 283, (1, 0, 1, 0, 0): 281, (1, 0, 0, 1, 0): 287, (1, 0, 0, 0, 0): 286,
    (0, 1, 1, 1, 0): 196, (0, 1, 1, 0, 0): 194, (0, 1, 0, 1, 0): 197, (0, 1, 0, 0, 0): 194,
    (0, 0, 1, 1, 0): 194, (0, 0, 1, 0, 0): 192, (0, 0, 0, 1, 0): 196, (0, 0, 0, 0, 0): 194,
}


def _is_instruction(line):
    return bool(line) and not line.startswith(('.', ';')) and not re.match(r'^\S+:', line)


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    """{(INTEG, FORCES, ZMU, REC, LOSS): lines of the kernel's body} from the assembly listing, built with the command `make` would run."""
    dry = subprocess.run(['make', '-C', CSRC, '-n', '-B', 'rollout_fwd_cp_fast.o'], capture_output=True, text=True, check=True).stdout
    cmd = [ln for ln in dry.split('\n') if 'rollout_fwd_cp_fast.hip' in ln and ' -c ' in ln]
    assert len(cmd) == 1, dry
    words = cmd[0].split()
    out = str(tmp_path_factory.mktemp('fwd_cp_listing') / 'rollout_fwd_cp_fast.s')
    words = words[:words.index('-c')] + ['--cuda-device-only', '-S', 'rollout_fwd_cp_fast.hip', '-o', out]
    subprocess.run(words, cwd=CSRC, check=True, capture_output=True)
    text = open(out).read()
    found = {}
    for m in re.finditer(r'^(_ZN2mf21rollout_fwd_cp_kernelIfLi(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)EE\w*):[^\n]*\n(.*?)\n\s+s_endpgm', text, re.S | re.M):
        found[tuple(int(v) for v in m.groups()[1:6])] = [ln.strip() for ln in m.group(7).split('\n')]
    assert set(found) == set(PARENT), sorted(set(found) ^ set(PARENT))
    return found


def _step_loops(lines):
    """Instruction counts (closing branch included) of the innermost loops of a hundred instructions or more: the step loops."""
    labels = {ln.split(':')[0]: i for i, ln in enumerate(lines) if re.match(r'^\.LBB\d+_\d+:', ln)}
    loops = []
    for i, ln in enumerate(lines):
        m = re.match(r's_c?branch\w* (\.LBB\d+_\d+)', ln)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i))
    inner = [(a, b) for a, b in loops if not any((c, d) != (a, b) and a <= c and d <= b for c, d in loops)]
    counts = [sum(1 for ln in lines[a:b + 1] if _is_instruction(ln)) for a, b in inner]
    return [c for c in counts if c >= 100]


def test_fit_step_forward_loop_is_within_its_budget(kernels):
    counts = _step_loops(kernels[FIT_STEP_FORWARD])
    print('fit step forward, instructions per two steps:', counts, 'parent', PARENT[FIT_STEP_FORWARD])
    assert len(counts) == 2, counts      # with and without a friction map
    assert max(counts) <= BUDGET, counts


def test_no_step_loop_grew(kernels):
    grown = []
    for key, lines in sorted(kernels.items()):
        counts = _step_loops(lines)
        print(key, counts, 'parent', PARENT[key])
        assert len(counts) == 2, (key, counts)
        if max(counts) > PARENT[key]:
            grown.append((key, counts, PARENT[key]))
    assert not grown, grown


def _vgprs(tok):
    m = re.match(r'^v\[(\d+):(\d+)\]', tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r'^v(\d+)\b', tok)
    return {int(m.group(1))} if m else set()


def test_inline_assembly_dpp_reads_keep_their_distance(kernels):
    """A VALU result read through DPP needs two wait states; the compiler pads its own DPP instructions and cannot see those in assembly
    text.  For each of them: the two wait states in front (an s_nop N is N + 1 of them) write none of the registers its DPP operand reads."""
    seen = 0
    for key, lines in kernels.items():
        in_asm = False
        for i, ln in enumerate(lines):
            if ln.startswith(';;#ASMSTART'):
                in_asm = True
            elif ln.startswith(';;#ASMEND'):
                in_asm = False
            if not (in_asm and _is_instruction(ln) and ('quad_perm' in ln or 'row_' in ln)):
                continue
            seen += 1
            ops = [t.strip() for t in ln.split(None, 1)[1].split(',')]
            src = _vgprs(ops[1])      # VOP2 DPP: vdst, src0 (the DPP operand), vsrc1
            assert src, ln
            waited, j = 0, i - 1
            while waited < 2 and j >= 0:
                prev = lines[j]
                j -= 1
                if not _is_instruction(prev):
                    assert not re.match(r'^\.LBB', prev), (key, i, 'a branch target inside the window', ln)
                    continue
                if prev.startswith('s_nop'):
                    waited += int(prev.split()[1]) + 1
                    continue
                waited += 1
                pops = prev.split(None, 1)
                dst = _vgprs(pops[1].split(',')[0].strip()) if len(pops) > 1 and pops[0].startswith('v_') else set()
                assert not (dst & src), (key, i, prev, ln)
    assert seen >= 2 * 2 * len(PARENT), seen      # two fused multiply-adds per step loop copy at least
