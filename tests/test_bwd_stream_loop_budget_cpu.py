"""Instruction budget of the streaming backward's loops (rollout_bwd_cp_kernel.h, MODE = kCpStream).  Each wave of a workgroup has a SIMD
to itself, so the length of its loop is what it costs -- though not at an issue slot per instruction: taking 36 of 309 instructions out
of the computing wave's loop shortened its busy time by 4 %, and the launch only followed when the fetching waves' loop shrank as well
(DESIGN.md section 8).  The listings of rollout_bwd_cp_stream_fast.hip and rollout_bwd_dyn_cp_stream_fast.hip, compiled with the
Makefile's own command lines, are held to
  * 268 instructions per trip (two steps, the closing branch included) in the computing loop of the fit step's backward
    <float, 1, true, false, kCpStream, 12, 3> -- 309 at the parent commit (b21fc5a), before the chain took its cross-lane operands inside
    the arithmetic instructions (rollout_cp_common.h: cp_rot_back, cp_colT, cp_cross_pair, cp_cell_terms), the ring was walked by a running
    byte offset, the wave's pending loads were waited for once in front of the loop (273) and the translation unit was scheduled for
    instruction-level parallelism (the only s_nop left in the loop are the two inside cp_colT); the floor that was asked for is 296;
  * no more than the parent's count in the computing loop of every other streaming kernel of the default integrator (PARENT below);
  * no more than the parent's 2031 in the fetching loop (nine steps) of the fit step's kernel;
  * the distance the compiler cannot check: a DPP instruction written as inline assembly reads its DPP operand no sooner than two wait
    states after the instruction that wrote it -- and a DPP instruction of the COMPILER's keeps that distance from a writer inside
    assembly text, which the compiler's hazard pass does not see as a vector write;
  * no scratch in any of the twelve float32 streaming kernels, and at most 256 registers in the six-slot positions-only ones."""
import os
import re
import shutil
import subprocess

import pytest

from tests.conftest import REPO

CSRC = os.path.join(REPO, 'monoforce_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc'
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which('make') is None, reason='needs hipcc and make')

UNITS = ('rollout_bwd_cp_stream_fast', 'rollout_bwd_dyn_cp_stream_fast')
FIT_STEP_BACKWARD = (1, 1, 0, 12, 3)
BUDGET, FLOOR_ASKED = 268, 296
FETCH_LOOP_PARENT = 2031
# (INTEG, XS_ONLY, GCTRL, SLOTS, BATCH) -> instructions of the computing loop per trip of two steps, closing branch included, at the parent
# commit (b21fc5a)
PARENT = {
    (1, 1, 0, 12, 3): 309, (1, 1, 0, 6, 2): 365,
    (1, 1, 1, 12, 3): 334, (1, 1, 1, 6, 2): 400,
    (1, 0, 0, 12, 3): 333, (1, 0, 0, 6, 3): 389,
    (1, 0, 1, 12, 3): 359, (1, 0, 1, 6, 3): 424,
}
DYNAMICS = {(0, xs, gc, 6, 3) for xs in (0, 1) for gc in (0, 1)}


def _is_instruction(line):
    return bool(line) and not line.startswith(('.', ';')) and not re.match(r'^\S+:', line)


@pytest.fixture(scope='module')
def listings(tmp_path_factory):
    """({key: lines of the kernel's body}, {key: metadata fields}) over both translation units, built with the commands `make` would run."""
    out_dir = tmp_path_factory.mktemp('bwd_stream_listing')
    procs = []
    for unit in UNITS:
        dry = subprocess.run(['make', '-C', CSRC, '-n', '-B', unit + '.o'], capture_output=True, text=True, check=True).stdout
        cmd = [ln for ln in dry.split('\n') if unit + '.hip' in ln and ' -c ' in ln]
        assert len(cmd) == 1, dry
        words = cmd[0].split()
        out = str(out_dir / (unit + '.s'))
        words = words[:words.index('-c')] + ['--cuda-device-only', '-S', unit + '.hip', '-o', out]
        procs.append((out, subprocess.Popen(words, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.PIPE)))
    sym = r'_ZN2mf21rollout_bwd_cp_kernelIfLi(\d)ELb(\d)ELb(\d)ELi3ELi(\d+)ELi(\d)ELb0ELb0ELb0EE\w*'
    bodies, meta = {}, {}
    for out, proc in procs:
        _, err = proc.communicate()
        assert proc.returncode == 0, err.decode()[-2000:]
        text = open(out).read()
        for m in re.finditer(r'^(' + sym + r'):[^\n]*\n(.*?)\n\s+s_endpgm', text, re.S | re.M):
            bodies[tuple(int(v) for v in m.groups()[1:6])] = [ln.strip() for ln in m.group(7).split('\n')]
        for m in re.finditer(r'\.name:\s+(' + sym + r')\n(.*?)\.wavefront_size', text, re.S):
            meta[tuple(int(v) for v in m.groups()[1:6])] = dict(re.findall(r'\.(\w+):\s+(\S+)', m.group(7)))
    assert set(bodies) == set(PARENT) | DYNAMICS, sorted(set(bodies) ^ (set(PARENT) | DYNAMICS))
    assert set(meta) == set(bodies)
    return bodies, meta


def _loops(lines):
    """(first line, last line, instructions -- closing branch included, has a global load) of every backward branch's span."""
    labels = {ln.split(':')[0]: i for i, ln in enumerate(lines) if re.match(r'^\.LBB\d+_\d+:', ln)}
    out = []
    for i, ln in enumerate(lines):
        m = re.match(r's_c?branch\w* (\.LBB\d+_\d+)', ln)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            a = labels[m.group(1)]
            body = [x for x in lines[a:i + 1] if _is_instruction(x)]
            out.append((a, i, len(body), any('global_load' in x for x in body)))
    return out


def _innermost(spans):
    return [s for s in spans if not any(t != s and s[0] <= t[0] and t[1] <= s[1] for t in spans)]


def _computing_loop(lines):
    """The innermost loop of >= 250 instructions without a global load (the wait for the ring inside it is a loop of five).  The kernels
    with control gradients hold a second such span behind it -- the out-of-line wait of the steps after the loop, which branches back --
    longer than the loop: the shortest is taken."""
    spans = _innermost([s for s in _loops(lines) if s[2] >= 250 and not s[3]])
    assert spans, 'no computing loop found'
    return min(s[2] for s in spans)


def _fetching_loop(lines):
    """The innermost loop of >= 250 instructions WITH global loads: three batches of three steps."""
    spans = _innermost([s for s in _loops(lines) if s[2] >= 250 and s[3]])
    assert len(spans) == 1, spans
    return spans[0][2]


def test_fit_step_backward_computing_loop_is_within_its_budget(listings):
    count = _computing_loop(listings[0][FIT_STEP_BACKWARD])
    print('fit step backward, computing loop, instructions per two steps:', count, 'parent', PARENT[FIT_STEP_BACKWARD])
    assert BUDGET <= FLOOR_ASKED
    assert count <= BUDGET, count


def test_no_computing_loop_grew(listings):
    grown = []
    for key in sorted(PARENT):
        count = _computing_loop(listings[0][key])
        print(key, count, 'parent', PARENT[key])
        if count > PARENT[key]:
            grown.append((key, count, PARENT[key]))
    assert not grown, grown


def test_fit_step_backward_fetching_loop_did_not_grow(listings):
    count = _fetching_loop(listings[0][FIT_STEP_BACKWARD])
    print('fit step backward, fetching loop, instructions per nine steps:', count, 'parent', FETCH_LOOP_PARENT)
    assert count <= FETCH_LOOP_PARENT, count


def _vgprs(tok):
    tok = tok.lstrip('-|')
    m = re.match(r'^v\[(\d+):(\d+)\]', tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r'^v(\d+)\b', tok)
    return {int(m.group(1))} if m else set()


def test_dpp_reads_keep_their_distance_from_inline_assembly(listings):
    """A VALU result read through DPP needs two wait states; the compiler pads between its own instructions only.  For every DPP instruction
    inside assembly text: the two wait states in front (an s_nop N is N + 1 of them) write none of the registers its DPP operand reads,
    and no branch target lies among them.  For every DPP instruction of the compiler's: no instruction INSIDE assembly text among the two
    wait states in front writes them."""
    inside, outside = 0, 0
    for key, lines in listings[0].items():
        in_asm, flags = False, []
        for ln in lines:
            if ln.startswith(';;#ASMSTART'):
                in_asm = True
            elif ln.startswith(';;#ASMEND'):
                in_asm = False
            flags.append(in_asm)
        for i, ln in enumerate(lines):
            if not (_is_instruction(ln) and ('quad_perm' in ln or 'row_' in ln)):
                continue
            ops = [t.strip() for t in ln.split(None, 1)[1].split(',')]
            src = _vgprs(ops[1])      # VOP1 / VOP2 DPP: vdst, src0 (the DPP operand)[, vsrc1]
            assert src, ln
            inside += flags[i]
            outside += not flags[i]
            waited, j = 0, i - 1
            while waited < 2 and j >= 0:
                prev = lines[j]
                j -= 1
                if not _is_instruction(prev):
                    if re.match(r'^\.LBB', prev):
                        assert not flags[i], (key, i, 'a branch target inside the window', ln)
                        break      # (the compiler's own instruction: what lies beyond the label is the compiler's to pad)
                    continue
                if prev.startswith('s_nop'):
                    waited += int(prev.split()[1]) + 1
                    continue
                waited += 1
                if not (flags[i] or flags[j + 1]):
                    continue
                pops = prev.split(None, 1)
                dst = _vgprs(pops[1].split(',')[0].strip()) if len(pops) > 1 and pops[0].startswith('v_') else set()
                assert not (dst & src), (key, i, prev, ln)
    # per step of the default integrator's chain: 3 x 2 (cp_rot_back) + 2 (cp_colT) + 2 x 2 (cp_cross_pair) + 1 (cp_cell_terms); a computing
    # loop holds two steps, a kernel at least one more step outside it
    assert inside >= 13 * 3 * len(PARENT), inside
    assert outside > inside


def test_streaming_kernels_use_no_scratch_and_keep_their_registers(listings):
    meta = listings[1]
    assert len(meta) == 12
    for key, fields in sorted(meta.items()):
        print(key, {k: fields.get(k) for k in ('vgpr_count', 'agpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')})
        assert int(fields['private_segment_fixed_size']) == 0, (key, fields['private_segment_fixed_size'])
        assert int(fields.get('vgpr_spill_count', 0)) == 0, key      # (scalar registers spill into lanes of a vector register: no memory)
        if key[:2] == (1, 1) and key[3] == 6:      # six-slot, positions only: two workgroups share a CU's four SIMDs
            assert int(fields['vgpr_count']) <= 256, (key, fields['vgpr_count'])
