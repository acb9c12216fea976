"""Which rollout kernel instantiations can a launch reach?  For machines WITHOUT a GPU.

    python tools/reachable_rollout_kernels.py [--out profiles/rollout_kernels_reachable.txt] [--jobs 8]

Without a device the entry points still validate, plan (rollout_route.hip assumes an MI355X) and dispatch; MF_KLAUNCH notes the kernel
stub, the launch fails cleanly (MF_ERR_LAUNCH) and `mf_last_launch()` names the instantiation.  This tool calls
mf_rollout_fwd_{f32,f64} and mf_rollout_bwd_{f32,f64} with ONE dummy host buffer behind every pointer, over

  * the descriptor grid of tests/test_rollout_routes_cpu.py (+-1 rollout of every threshold, bodies of 1 .. 513 points, every
    points_per_lane, both integrators, both math modes, shared and per-rollout maps, joints), each row with force_stride as the row
    has it and as mf_rollout_force_stride answers,
  * crossed with the buffer combinations FwdBits / BwdBits distinguish (forces, Xraw, rec, zmu / zmu_scratch / mu, cost rows with
    cost_project 0 / 1, gcontrols, positions-only / all six upstreams, MfRolloutLoss in each form),
  * once per switch setting of SWITCHES below, in child processes (the library reads a switch once per process),

and writes the sorted set of names.  A launch that goes out in chunks notes its last chunk only: the same kernel as the others.
With a device present the dummy pointers would be dereferenced by real kernels, so the tool asks the HIP runtime for the device
count first and refuses to go on if any device answers.  Not a test; nothing under tests/ or bench.py runs it.

The part of the output file from the line that starts with KEPT on is kept as it is when the file is rewritten: the kernels that stay
in the build although the sweep does not reach them, with the reason (tests/test_rollout_instances_cpu.py reads both parts)."""
import argparse
import ctypes as C
import itertools
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, 'profiles', 'rollout_kernels_reachable.txt')
KEPT = '## kept, not reached by the sweep'

MF_ERR_LAUNCH = 3
# the default, the switches of tests/test_rollout_routes_cpu.py, and those that change the form of a launch
EXTRA_SWITCHES = ('MF_CP_BWD_MODE=0', 'MF_CP_BWD_MODE=1', 'MF_MW_TILE=0', 'MF_BWD_XS_ZMU=0', 'MF_BWD_XS_PPL=0', 'MF_CP_BWD_ZMU=0',
                  'MF_CP_BLOCK=256')


def switches():
    from tests.test_rollout_routes_cpu import SWITCHES
    return ('',) + tuple(SWITCHES) + EXTRA_SWITCHES


def _bufs(cls, names, p):
    b = cls()
    for n in names:
        setattr(b, n, p)
    return b


def fwd_variants(lib, p, joints):
    """[(MfRolloutFwdBufs, cost_project, whether Fs / Ff are there)]: every combination of optional buffers the forward's planner tells apart."""
    out, keep = [], []
    base = ('z', 'controls', 'ts', 'points', 'part', 'x0', 'xd0', 'R0', 'w0', 'Xs', 'Rs') + (('joint_angles',) if joints else ())
    maps = [m + z for m in ((), ('mu',)) for z in ((), ('zmu_scratch',), ('zmu',))]
    losses = [None]
    for flags, fields in ((0, ('gt', 'row_w', 'partial', 'ticket', 'loss')), (lib.MF_LOSS_VALUE_IN_BACKWARD, ('loss',))):
        L = _bufs(lib.MfRolloutLoss, fields, p)
        L.T2, L.flags = 10, flags
        losses.append(L)
    keep.extend(losses)
    for forces, rec, m, L in itertools.product((False, True), ((), ('rec',)), maps, losses):
        b = _bufs(lib.MfRolloutFwdBufs, base + ('Xds', 'Omegas') + (('Fs', 'Ff') if forces else ()) + rec + m, p)
        if L is not None:
            b.loss = C.cast(C.pointer(L), C.c_void_p)
        out.append((b, 0, forces))
    # (Xraw and path_cost are tested by the kernels, not by the planner: crossed with forces / rec and with cost_project only)
    for forces, rec in itertools.product((False, True), ((), ('rec',))):
        out.append((_bufs(lib.MfRolloutFwdBufs, base + ('Xds', 'Omegas', 'Xraw') + (('Fs', 'Ff') if forces else ()) + rec, p), 0, forces))
    for project, m in itertools.product((0, 1), maps):      # cost rows: only Xs and Rs beside them
        out.append((_bufs(lib.MfRolloutFwdBufs, base + ('cost_rows',) + (('path_cost',) if project else ()) + m, p), project, False))
    return out, keep


def bwd_variants(lib, p, joints):
    """[MfRolloutBwdBufs]: every combination of optional buffers the backward's planner tells apart."""
    out, keep = [], []
    base = ('z', 'controls', 'ts', 'points', 'part', 'x_init', 'xd0', 'R0', 'w0', 'Xraw', 'Xds', 'Rs', 'Omegas', 'zeros',
            'gz', 'gmu', 'gx0', 'gxd0', 'gR0', 'gw0') + (('joint_angles', 'gjoint_angles') if joints else ())
    maps = [m + z for m in ((), ('mu',)) for z in ((), ('zmu_scratch',), ('zmu',))]
    ups = [('gXs',), ('gXs', 'gXds', 'gRs', 'gOmegas', 'gFs', 'gFf'), ()]
    rows = ('gt', 'near', 'w', 'row_stamp', 'row_w', 'gloss', 'Xs')
    for flags, fields in ((0, rows), (lib.MF_LOSS_VALUE_IN_BACKWARD, rows + ('partial', 'ticket', 'loss'))):
        L = _bufs(lib.MfRolloutLoss, fields, p)
        L.T2, L.flags = 10, flags
        keep.append(L)
        ups.append(L)
    for up, rec, gc, m in itertools.product(ups, ((), ('rec',)), ((), ('gcontrols',)), maps):
        b = _bufs(lib.MfRolloutBwdBufs, base + (up if isinstance(up, tuple) else ()) + rec + gc + m, p)
        if not isinstance(up, tuple):
            b.loss = C.cast(C.pointer(up), C.c_void_p)
        out.append(b)
    return out, keep


def sweep():
    """The names this process's switch setting reaches, over the whole grid."""
    from monoforce_amd import _lib
    from tests.test_rollout_routes_cpu import FIELDS, grid
    L = _lib.lib()
    n = C.c_int(-1)
    rc = L.hipGetDeviceCount(C.byref(n))      # (the runtime the library itself is bound to)
    if rc == 0 and n.value > 0:
        sys.exit(f'{n.value} GPU(s) answer: this sweep hands dummy host pointers to the entry points and must not launch -- run it on a machine without one')
    raw = C.create_string_buffer(1 << 16)
    p = C.c_void_p((C.addressof(raw) + 63) & ~63)
    variants = {j: (fwd_variants(_lib, p, j), bwd_variants(_lib, p, j)) for j in (0, 1)}
    entry = [(L.mf_rollout_fwd_f32, L.mf_rollout_fwd_f64), (L.mf_rollout_bwd_f32, L.mf_rollout_bwd_f64)]
    last, stride = L.mf_last_launch, L.mf_rollout_force_stride
    names = set()
    for r in grid().tolist():
        d = _lib.MfRolloutDesc(**dict(zip(FIELDS, r)))
        d.n_tracks = 4 if d.has_joints else 2
        d.pose_stride = 1
        d.mass, d.gravity, d.stiffness, d.damping, d.grid_res, d.d_max, d.dt, d.robot_size_y = 40., 9.81, 5000., 500., .1, 6.4, .01, .6
        dref = C.byref(d)
        (fwd, _), (bwd, _) = variants[d.has_joints]
        strides = sorted({d.force_stride, max(d.force_stride, stride(dref))})
        for f, fs in itertools.product(entry[0], strides):
            d.force_stride = fs
            for b, project, forces in fwd:
                if forces and fs != strides[-1]:
                    continue      # (force rows narrower than the lane map are refused: those variants at the wider stride only)
                d.cost_project = project
                if f(dref, C.byref(b), None) == MF_ERR_LAUNCH:
                    names.add(last())
        d.force_stride, d.cost_project = strides[0], 0
        for f in entry[1]:
            for b in bwd:
                if f(dref, C.byref(b), None) == MF_ERR_LAUNCH:
                    names.add(last())
    return sorted({s.decode().split(' grid=')[0] for s in names})


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--jobs', type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.child:
        print('\n'.join(sweep()))
        return 0
    todo, running, reached = list(switches()), [], {}
    while todo or running:
        while todo and len(running) < args.jobs:
            s = todo.pop(0)
            env = dict(os.environ, **dict([s.split('=')] if s else []))
            running.append((s, subprocess.Popen([sys.executable, os.path.abspath(__file__), '--child'], env=env, stdout=subprocess.PIPE, text=True)))
        s, proc = running.pop(0)
        out = proc.communicate()[0]
        if proc.returncode:
            sys.exit(f'the sweep under "{s or "default"}" failed')
        reached[s] = set(filter(None, out.split('\n')))
        print(f'{s or "(default)":32s} {len(reached[s]):4d} kernels', file=sys.stderr)
    names = sorted(set().union(*reached.values()))
    kept = ''
    if os.path.exists(args.out):
        text = open(args.out).read()
        if KEPT in text:
            kept = text[text.index(KEPT):]
    with open(args.out, 'w') as f:
        f.write('# The rollout kernel instantiations a launch can reach: tools/reachable_rollout_kernels.py on a machine without a GPU (an MI355X\n'
                '# is assumed: 256 CUs; the thresholds scale with the CU count, which moves the batch size a (family, lane map) pair is chosen at,\n'
                '# not which pairs exist).  Settings swept: default, ' + ', '.join(filter(None, reached)) + '.\n'
                f'# {len(names)} kernels.\n')
        f.write('\n'.join(names) + '\n')
        f.write(kept)
    print(f'{args.out}: {len(names)} reachable kernels', file=sys.stderr)
    return 0


if __name__ == '__main__':
    sys.exit(main())
