"""A/B of the component-parallel backward between two builds of the library, at the shapes that route to its kernels: per integrator
and 256 / 1024 / 2048 (streaming, 12 and 6 slots) / 4096 (record-reading, interleaved maps) / 8192 (early recompute, window, fused loss)
rollouts, the median and minimum backward kernel time (HIP events around the C-ABI launch, AB_N = 24 launches after 3 warm-up steps) of
  fit  -- the terrain-fit step (positions-only, fused physics loss): the XS_ONLY kernels, and
  full -- a backward through all six outputs with control gradients,
with the kernel mf_last_launch() names.  One process per library (it is loaded once); alternate them and time the yardstick twice --
the spread between its two runs is the noise:

    MONOFORCE_HIP_LIB=<parent .so> python tools/ab_bwd_cp_lib.py parent1 > p1.txt
    MONOFORCE_HIP_LIB=<new .so>    python tools/ab_bwd_cp_lib.py new1    > n1.txt
    MONOFORCE_HIP_LIB=<parent .so> python tools/ab_bwd_cp_lib.py parent2 > p2.txt
    MONOFORCE_HIP_LIB=<new .so>    python tools/ab_bwd_cp_lib.py new2    > n2.txt
    python tools/ab_bwd_cp_lib.py --table p1.txt p2.txt n1.txt n2.txt

(profiles/bwd_cp_split_ab.txt is the table of such a run.)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from bench import build_problem
from monoforce_amd import _timing, synthetic as syn
from monoforce_amd.train import TerrainFitProblem
DEV = 'cuda'
N = int(os.environ.get('AB_N', '24'))


def timed(fn):
    for _ in range(3):
        fn()
    _timing.start()
    for _ in range(N):
        fn()
    names = _timing.launches()
    rec = _timing.stop()
    out = []
    for k, v in rec.items():
        if 'bwd' in k:
            out.append((k, float(np.median(v)), float(np.min(v)), names.get(k, '')[:150]))
    return out


def table(p1, p2, n1, n2):
    """spread = |parent run 1 - parent run 2|, diff = mean(new) - mean(parent), per case of the four runs' `AB` lines."""
    import re

    def load(f):
        d = {}
        for ln in open(f):
            m = re.match(r'AB \S+ (integ=\d B=\d+ \w+) (\S+) med=(\S+) min=(\S+) (.*)', ln)
            if m and 'rollout_bwd' in m.group(2):
                d[m.group(1)] = (float(m.group(3)), m.group(5).split(' grid')[0].replace('mf::rollout_bwd_cp_kernel', ''))
        return d
    p1, p2, n1, n2 = load(p1), load(p2), load(n1), load(n2)
    print('case                     parent1 parent2  new1    new2    spread    diff         kernel')
    for k in p1:
        sp, pm, nm = abs(p1[k][0] - p2[k][0]), (p1[k][0] + p2[k][0]) / 2, (n1[k][0] + n2[k][0]) / 2
        flag = 'SLOWER' if nm - pm > sp else ('faster' if pm - nm > sp else 'inside')
        print(f'{k:24s} {p1[k][0]:.4f}  {p2[k][0]:.4f}  {n1[k][0]:.4f}  {n2[k][0]:.4f}  {sp:.4f}  {nm - pm:+.4f} ({(nm - pm) / pm * 100:+5.1f} %) {flag:7s} {p1[k][1]}')


def run(tag):
    for integ in (1, 0):
        for B in (256, 1024, 2048, 4096, 8192):
            cfg, dp, pts, masks, z, mu, ctrl = build_problem(B, 500, 4, DEV, integ)
            cd = ctrl.to(DEV)
            zl, ml = z.to(DEV).clone().requires_grad_(True), mu.to(DEV).clone().requires_grad_(True)
            prob = TerrainFitProblem(dp, syn.bump_terrain(syn.bump_params(100), 6.4, 0.05).to(DEV), mu.to(DEV), cd)
            for k, med, mn, name in timed(lambda: prob.step(zl, ml, eager=True)):
                print(f'AB {tag} integ={integ} B={B} fit {k} med={med:.4f} min={mn:.4f} {name}', flush=True)
            cl = cd.clone().requires_grad_(True)

            def full():
                zl.grad = ml.grad = cl.grad = None
                (Xs, Xds, Rs, Om), (Fs, Ff) = dp(zl.unsqueeze(0), cl, friction=ml.unsqueeze(0))
                ((Xs ** 2).mean() + (Xds ** 2).mean() + (Rs ** 2).mean() + (Om ** 2).mean() + 1e-6 * ((Fs ** 2).mean() + (Ff ** 2).mean())).backward()
            for k, med, mn, name in timed(full):
                print(f'AB {tag} integ={integ} B={B} full {k} med={med:.4f} min={mn:.4f} {name}', flush=True)
            del prob, dp, zl, ml, cl
            torch.cuda.empty_cache()


if __name__ == '__main__':
    if sys.argv[1] == '--table':
        table(*sys.argv[2:6])
    else:
        run(sys.argv[1])
