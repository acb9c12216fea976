#!/usr/bin/env python3
"""bench.py -- rollout-steps/s of the DPhysics hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run does what its headline figure needs and nothing else: it sets up the workload, warms up, chooses the launch mode,
times the K steps and prints the result line (the contract's keys, `config`; no detail file).  `--full` adds everything else
this script measures -- `roofline` with its per-kernel HIP-event figures, `comm_ms`, `forward_only`, the sweeps, the side
workloads, `cpu_baseline` and the detail file -- as described below.  `--dump-outputs DIR` writes what the timed path computed
in its LAST timed step, as a caller of that path receives it, to DIR/<name>.npy (float32 / float64, at most 64 MB in all; see
`dump_outputs`): the inputs are seeded, so two builds run with the same arguments can be compared output for output.

N > 1: one rank per GPU over RCCL.  Either the caller launches the ranks (`python -m torch.distributed.run --nproc-per-node N
... bench.py --gpus N`, RANK / LOCAL_RANK / WORLD_SIZE in the env) or, when WORLD_SIZE is absent, bench.py re-executes itself
under torch.distributed.run with N ranks.  It never runs fewer ranks than asked for: WORLD_SIZE != N, or fewer than N
visible GPUs, is an error (exit code 2).

A "step" is one pass of the hot path over one batch of synthetic input: B rollouts x T Euler steps x N contact points on a
256x256 terrain.  `value` = (B * T * world_size * K) / wall time of the K timed steps (barrier + synchronize on both sides,
max over ranks), inputs resident in HBM, outputs allocated inside the timed region (the API returns fresh tensors) or, when
the step is replayed as a hipGraph, owned by the captured graph.  Launch mode (`config.launch`): after the warm-up the step is
timed both ways on the host at hand -- launched call by call, and captured once and replayed as ONE hipGraph launch per step
(same kernels, same work) -- and the timed region runs in the faster mode; MF_BENCH_NO_GRAPH=1 keeps it launch by launch.
Kernel durations for `roofline` (--full) come from HIP events around the C-ABI launches of every 32nd timed step and of four steps run right after the region (those steps run
launch by launch in either mode).
Rollouts are independent: ranks shard the batch with no data-path collective (weak scaling: B rollouts per GPU); the
backward all-reduces the gradient of what the ranks SHARE -- one terrain / friction map pair, the same on every rank
(same seed), fitted to every rank's rollouts -- over RCCL.

Workloads (`--workload`; the default, c3, is BASELINE configs[2], the shape north_star quotes the metric on):
  c1   BASELINE configs[0]   1 rollout x 200 steps, 128x128 terrain (res 0.1), forward + backward
  c2   BASELINE configs[1]   256 rollouts x 500 steps, forward
  c3   BASELINE configs[2]   1024 rollouts x 500 steps x 4 contact points, forward + physics loss + backward to terrain
  c3f  the same batch, forward only (all six outputs written)
  c4   BASELINE configs[3]   TerrainEncoder (4 cams 3x256x512 -> 256x256 BEV) + 1024 rollouts, end-to-end train step
  c5   BASELINE configs[4]   8192 rollouts in total + encoder, sharded over the ranks (STRONG scaling: 8192 / N per GPU)

OUTPUT.  The LAST stdout line (rank 0) is ONE compact JSON object, < 4 KB (`compact_line`): the contract's keys, `config` and, with
--full, `roofline` (bound, achieved, peak, unit, frac, traffic, frac_traffic, frac_model, kernel, kernel_ms, ...), `cpu_baseline`
(value, unit, cores, kind, sample), `forward_only` and one ms-per-step number per side workload.  Everything else -- per-kernel
tables, the batch sweep, side workloads, CPU legs, kernel-instance strings -- goes to the DETAIL file of a --full run (`--detail`,
default bench_detail.json next to this script); the line names it under `detail`.  (Round 5 printed all of it as one 28.8 KB
line, too long to be parsed: tests/test_bench_line_cpu.py holds the line to its size now.)

The detail record (--full) carries, besides the contract's keys:
  roofline      dominant hand-written kernel of the headline step -- algorithmic bytes per launch (80 + 56 N
                bytes per rollout-step forward, 160 + 120 N backward) / its average launch duration, measured live with HIP
                events on the launch stream, against the 8 TB/s HBM peak -- plus `per_kernel` (forward AND backward
                fractions) and `batch_sweep` (forward / backward kernel at 1024, 4096, 8192, 16384 rollouts; `first_B_at_40pct`).
                `traffic` = HBM bytes per launch from rocprofv3 PMC passes of this command, read from
                profiles/hbm_traffic.json (`traffic_source` says so: it is not re-measured inside the run).
  forward_only  the c3f workload, same accounting (top level: both the forward-only and the forward+backward rate count)
  cpu_baseline  the CPU oracle (oracle/dphysics_oracle.py, a torch-CPU port of the reference algorithm) timed on this box's
                host cores on bounded samples: forward (no_grad), the autograd forward+backward of config 3, and config 1.
  other_workloads  (--full) short runs of c1, c2, c4 and `shoot` (trajectory shooting of 16384 sampled control
                sequences through the kernel's path-cost mode); N > 1: `strong_c3` (8192 rollouts in total) and c5.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: 8 TB/s HBM3E peak (~6.3 TB/s achievable)
EVENT_EVERY = 32             # kernel durations: HIP events around the launches of every 32nd step of the timed region (+ sampled steps after it)

WORKLOADS = {
    'c1': dict(B=1, T=200, N=4, backward=True, grid_res=0.1, desc='BASELINE configs[0]: 1 rollout x 200 steps, 128x128 terrain, forward + backward'),
    'c2': dict(B=256, T=500, N=4, backward=False, desc='BASELINE configs[1]: 256 rollouts x 500 steps, forward'),
    'c3f': dict(B=1024, T=500, N=4, backward=False, desc='north_star shape: 1024 rollouts x 500 steps x 4 points, forward only'),
    'c3': dict(B=1024, T=500, N=4, backward=True, desc='BASELINE configs[2]: 1024 rollouts x 500 steps, forward + physics loss + backward to terrain'),
    'c4': dict(B=1024, T=500, N=4, backward=True, encoder=True,
               desc='BASELINE configs[3]: TerrainEncoder (4 cams 3x256x512 -> 256x256 BEV) + 1024 rollouts per GPU, end-to-end train step'),
    # the same step as a real train.py loop sees it: a NEW image augmentation every step (terrain_encoder/utils.py:110-133 samples
    # resize / crop per sample), so the voxel plan of the splat is rebuilt in every forward instead of being served from the rig cache
    'c4_aug': dict(B=1024, T=500, N=4, backward=True, encoder=True, augment=True,
                   desc='BASELINE configs[3] with a fresh image augmentation (post_rots, post_trans) every step: the splat plan is rebuilt per forward'),
    # the reference's own operating point (examples/diff_physics.ipynb:199-226: 64 rollouts x 600 steps of the 223-point `marv` body on a
    # 128 x 128 grid -- the only timing the reference records) and two more body sizes of its robots
    'ref_nb': dict(B=64, T=600, N=223, backward=True, grid_res=0.1,
                   desc='the reference notebook shape (examples/diff_physics.ipynb:199-226): 64 rollouts x 600 steps x 223 contact points, 128x128 grid'),
    'n32': dict(B=1024, T=500, N=32, backward=True, desc='1024 rollouts x 500 steps x 32 contact points'),
    'n175': dict(B=64, T=500, N=175, backward=True, desc='64 rollouts x 500 steps x 175 contact points (tradr-sized body; open3d down-sampling itself unpinned)'),
    'c5': dict(B=8192, T=500, N=4, backward=True, encoder=True, strong=True,
               desc='BASELINE configs[4]: 8192 rollouts in total + encoder (one 4-camera sample per GPU), data-parallel with RCCL gradient all-reduce'),
}


def fwd_bytes_per_rollout_step(N):
    """controls 8 + states written 72 + forces written 24 N + map cells gathered 32 N."""
    return 80 + 56 * N


def bwd_bytes_per_rollout_step(N):
    """upstream grads 72 + 24 N, controls 8, saved state 72, re-gather 32 N, scatter RMW 64 N, grad-controls 8."""
    return 160 + 120 * N


# The same model restricted to what must cross HBM: SURVEY 8d counts the 32 N bytes of gathered map cells (and, backward, the 64 N of
# scatter read-modify-writes) "even when served from LDS / L2" -- the maps of these workloads are 512 KiB and their gradient copies a
# few MB, resident in every XCD's L2 / the memory-side cache.  `frac_hbm` next to every `frac` is computed on these bytes, so that
# a fraction near (or above) the achievable 6.3 TB/s is not read as HBM bandwidth it is not.
def fwd_hbm_bytes_per_rollout_step(N, forces=True):
    """controls 8 + states 72 (+ forces 24 N when written): no map cells."""
    return 80 + (24 * N if forces else 0)


def bwd_hbm_bytes_per_rollout_step(N):
    """upstream grads 72 + 24 N, controls 8, saved state 72, grad-controls 8: no map cells, no scatter RMW."""
    return 160 + 24 * N


def fwd_states_only_bytes_per_rollout_step(N):
    """A states-only forward (FORCES = false: the fit / train steps discard the forces) is asked to move
    controls 8 + states 72 + map cells 32 N -- NOT the 24 N of forces: its `algorithmic_bytes` is 80 + 32 N (208 B at N = 4)."""
    return 80 + 32 * N


def parse_instance(text):
    """'mf::rollout_bwd_kernel<float, 4, 1, 1, true, ...> grid=.. block=.. launches=..' -> ('rollout_bwd_kernel', ['float', '4', ...], {'grid': .., 'block': ..})."""
    import re
    m = re.match(r'\s*(?:mf::)?(\w+)<(.*?)>(.*)$', text or '')
    if not m:
        return None, [], {}
    kv = {k: int(v) for k, v in re.findall(r'(\w+)=(\d+)', m.group(3))}
    return m.group(1), [t.strip() for t in m.group(2).split(',')], kv


def instance_bytes_per_rollout_step(instance, N, T=500, T2=50):
    """The bytes THIS kernel instantiation is asked to move per rollout-step -- SURVEY 8d's figure with the rows the
    instantiation never touches taken out and the ones it adds (the forward's record) put in -- and the terms, as text.  Returns
    (bytes, text, flags) or (None, reason, {}) for an unknown kernel.  Template parameter order: the kernels' headers
    (rollout_bwd_kernel.h:890, rollout_bwd_cp_kernel.h:61, rollout_bwd_mw_kernel.h:62, rollout_fwd_kernel.h:226, rollout_fwd_cp_kernel.h:16)."""
    name, t, _ = parse_instance(instance)
    if name is None:
        return None, 'no kernel instance recorded', {}
    b = lambda i, default=False: (t[i] == 'true') if i < len(t) else default      # noqa: E731
    terms, flags = [], {}
    if name in ('rollout_bwd_kernel', 'rollout_bwd_cp_kernel', 'rollout_bwd_mw_kernel'):
        if name == 'rollout_bwd_kernel':       # <S, G, PPL, INTEG, FAST, JOINTS, CARRY, XS_ONLY, ZMU, WIN, LOSS>
            xs, win, loss, rec, gctrl = b(7), b(9), b(10), 0, True
        elif name == 'rollout_bwd_cp_kernel':  # <S, INTEG, XS_ONLY, GCTRL, MODE, SLOTS, BATCH, ZMU, WIN, ONE1>
            xs, gctrl, mode, win, loss = b(2), b(3), int(t[4]), b(8), b(9)      # (kCpStream's fused loss is a launch argument, not an instantiation)
            rec = 256 if mode >= 2 else 0      # kCpSaved / kCpStream read the forward's 16-byte quad per lane, 16 lanes per rollout
        else:                                  # <S, G, XS_ONLY, TILE, INTEG>
            xs, gctrl, win, loss, rec = b(2), True, int(t[3]) > 0, False, 16
        total = 0
        if xs:
            total += 12; terms.append('positions-only upstream: one 12-B row (dL/dXs, or the Xs row a fused loss reads)')
        else:
            total += 72 + 24 * N; terms.append(f'upstream rows 72 + 24 N = {72 + 24 * N}')
        if loss:
            total += 12 * T2 / T; terms.append(f'ground-truth rows 12 B x {T2}/{T} stamped steps')
        total += 8 + 72; terms.append('controls 8 + saved state 72')
        total += 32 * N; terms.append(f're-gathered cells 32 N = {32 * N} (L2 / LDS-served)')
        total += 64 * N; terms.append(f'cell-gradient read-modify-write 64 N = {64 * N}' + (' (LDS window first)' if win else ' (L2 atomics)'))
        if gctrl:
            total += 8; terms.append('control gradient 8')
        if rec:
            total += rec; terms.append(f"the forward's record {rec}")
        flags = dict(xs_only=xs, win=win, fused_loss=loss, record=rec)
        return total, ' + '.join(terms), flags
    if name in ('rollout_fwd_kernel', 'rollout_fwd_cp_kernel'):
        if name == 'rollout_fwd_kernel':       # <S, G, PPL, INTEG, FAST, JOINTS, FORCES, COST, SPLIT, ZMU, REC>
            forces, cost, rec = b(6, True), int(t[7]) if len(t) > 7 else 0, 16 if b(10) else 0
        else:                                  # <S, INTEG, FORCES, ZMU, REC, LOSS>
            forces, cost, rec = b(2, True), 0, 256 if b(4) else 0
        if cost:
            return 8 + 16 + 32 * N, f'path-cost mode: controls 8 + cost row 16 + cells 32 N = {32 * N}', dict(cost=True)
        total = 8 + 72 + 32 * N
        terms = ['controls 8 + states 72', f'gathered cells 32 N = {32 * N} (L2-served)']
        if forces:
            total += 24 * N; terms.append(f'force rows 24 N = {24 * N}')
        if rec:
            total += rec; terms.append(f'the record kept for the backward {rec}')
        return total, ' + '.join(terms), dict(forces=forces, record=rec)
    return None, f'no byte model for {name}', {}


def regime_of(instance, B, N):
    """What bounds this launch, from its occupancy (MI355X: 1024 SIMDs) and the counters on file -- stated, not inferred from `frac`:
    below one wave per SIMD a launch costs what ONE wave's dependent chain issues (profiles/r3_critical_path.txt); the saturated
    positions-only backward is VALU-bound (profiles/r5h_pmc_backward_sat_B32768.txt: VALUs ~92 % busy, 1.5 TB/s at the HBM counters)."""
    name, t, kv = parse_instance(instance)
    if name is None:
        return None
    waves = kv.get('grid', 0) * max(kv.get('block', 64) // 64, 1)
    per_simd = waves / 1024.0
    if per_simd < 1.0:
        return f'issue-bound: {per_simd:.2f} waves per SIMD, a step costs what one wave\'s dependent chain issues'
    if name in ('rollout_bwd_cp_kernel', 'rollout_fwd_cp_kernel'):
        return (f'{per_simd:.1f} waves per SIMD of the component-parallel kernel: ' +
                ('VALU-bound (the recomputing form at two waves per SIMD)' if per_simd >= 2.0 else 'one dependent chain per SIMD + the CU\'s shared L1 address path (DESIGN 8)'))
    if name == 'rollout_bwd_kernel' and len(t) > 7 and t[7] == 'true':
        return f'VALU-bound ({per_simd:.1f} waves per SIMD; PMC: VALUs ~92 % busy at two waves per SIMD); cells and RMW are cache / LDS-served'
    if name == 'rollout_fwd_kernel':
        return f'{per_simd:.1f} waves per SIMD: bound by the CU\'s L1 address path (gathers) and the output stores'
    return f'{per_simd:.1f} waves per SIMD'


def build_problem(B, T, N, device, integ, seed=0, grid_res=0.05, terrain_seed=0):
    """Synthetic inputs: terrain / friction from `terrain_seed`, controls from `seed`."""
    from monoforce_amd import synthetic as syn
    from monoforce_amd.dphys_config import DPhysConfig
    from monoforce_amd.dphysics import DPhysics
    if N == 4:
        pts, masks = syn.robot_points_4()
    else:
        pts, masks = syn.robot_points_box(N, seed=1, n_tracks=2)
    cfg = DPhysConfig(robot='tradr', grid_res=grid_res, robot_points=pts, driving_parts=masks)
    cfg.use_odeint = (integ == 1)
    if T > int(cfg.traj_sim_time / cfg.dt):
        cfg.traj_sim_time = T * cfg.dt + 1e-9      # a longer horizon than the default 5 s (the notebook's 6 s)
    z = syn.bump_terrain(syn.bump_params(terrain_seed), 6.4, grid_res)
    mu = syn.wave_friction(6.4, grid_res)
    ctrl = syn.const_controls(B, T, seed=seed)
    dp = DPhysics(cfg, device=device) if device is not None else None
    return cfg, dp, pts, masks, z, mu, ctrl


def _oracle_spec(cfg, pts, masks, integ, grid_res):
    from oracle import dphysics_oracle as orc      # checker / baseline only -- never on the product path
    return orc.RolloutSpec(points=torch.as_tensor(pts), driving_parts=[torch.as_tensor(m) for m in masks],
                           robot_size_y=float(cfg.robot_size[1]), mass=cfg.robot_mass, grid_res=grid_res, d_max=6.4,
                           integrator=integ)


def _time_cpu(fn, budget_s, max_runs=12):
    """Median run time within a time budget; the first run is a warm-up unless it alone used up half the budget."""
    times, t_start = [], time.perf_counter()
    while not times or (time.perf_counter() - t_start < budget_s and len(times) < max_runs):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
        if len(times) == 1 and times[0] > budget_s / 2:
            return times[0], 1
    kept = times[1:] if len(times) > 1 else times
    return float(np.median(kept)), len(kept)


def _best_threads(fn, candidates):
    """The torch intra-op thread count at which `fn` runs fastest on this host (one run each after a warm-up): the oracle's tensors are small
    ([B, N, 3] at a few hundred rollouts), and all 128 threads of a GPU box's host run it several times SLOWER than 8 do (round 6: the GPU
    test tier's oracle calls 91 s -> 18 s).  The baseline is timed at the best count found, and says which."""
    keep = torch.get_num_threads()
    best = (float('inf'), keep)
    try:
        for i, n in enumerate(candidates):
            torch.set_num_threads(n)
            if i == 0:
                fn()
            t0 = time.perf_counter()
            fn()
            best = min(best, (time.perf_counter() - t0, n))
    finally:
        torch.set_num_threads(keep)
    return best[1]


def cpu_baseline(N, integ, T, budget_s=12.0, headline='c3'):
    """Time the CPU oracle on bounded samples, host threads as torch sees them.  `value` is the leg that does the SAME work as the
    GPU headline beside it: for c3 the autograd forward + backward of config 3 on a B = 32 sample of its 1024 rollouts
    (rollout-steps/s of that sample; its cost per rollout GROWS with B -- every gather's autograd node materialises a [B,H,W]
    gradient, as in the reference -- so the sample flatters the CPU); for a forward-only headline the no_grad forward at B = 256.
    The other legs stay under `legs`: `c2_forward`, `c3_autograd`, `c1_forward` (config 1 at its own size)."""
    from oracle import dphysics_oracle as orc      # checker / baseline only -- never on the product path
    from monoforce_amd import synthetic as syn
    all_threads = torch.get_num_threads()
    cand = sorted({min(8, all_threads), min(32, all_threads), all_threads})
    legs = {}
    # forward, no_grad (C2)
    Bs = 256
    cfg, _, pts, masks, z, mu, ctrl = build_problem(Bs, T, N, None, integ, seed=0)
    spec = _oracle_spec(cfg, pts, masks, integ, 0.05)
    zb, mb = z.unsqueeze(0).expand(Bs, -1, -1), mu.unsqueeze(0).expand(Bs, -1, -1)

    def fwd():
        with torch.no_grad():
            orc.rollout(spec, zb, ctrl, friction=mb)
    cores = _best_threads(fwd, cand)
    torch.set_num_threads(cores)
    t, n = _time_cpu(fwd, budget_s)
    legs['c2_forward'] = dict(value=Bs * T / t, unit='rollout-steps/s', cores=cores, kind='port',
                              sample=f'oracle/dphysics_oracle.py (torch-CPU port), B={Bs} x T={T} x N={N}, 256x256 shared map, forward '
                                     f'no_grad, median of {n} runs')
    # forward + autograd backward to the terrain (C3), loss on every 10th pose like physics_loss
    Ba = 32       # every gather's autograd node materialises a [B,H,W] gradient (as in the reference): time grows with B^2
    ctrl_a = syn.const_controls(Ba, T, seed=0)

    def fwd_bwd():
        zl = z.clone().requires_grad_(True)
        ml = mu.clone().requires_grad_(True)
        (Xs, _, _, _), _ = orc.rollout(spec, zl.unsqueeze(0).expand(Ba, -1, -1), ctrl_a, friction=ml.unsqueeze(0).expand(Ba, -1, -1))
        (Xs[:, 9::10] ** 2).mean().backward()
    cores = _best_threads(fwd_bwd, cand)
    torch.set_num_threads(cores)
    t, n = _time_cpu(fwd_bwd, 2.0 * budget_s, max_runs=5)       # (one run is 2 .. 7 s depending on the thread count)
    legs['c3_autograd'] = dict(value=Ba * T / t, unit='rollout-steps/s', cores=cores, kind='port',
                               sample=f'oracle/dphysics_oracle.py (torch-CPU port), B={Ba} (a sample of config 3\'s 1024 rollouts: the autograd graph of one '
                                      f'run holds a [B,H,W] gradient per gather, time per rollout grows with B) x T={T} x N={N}, 256x256 shared map, forward + torch '
                                      f'autograd backward to terrain and friction, median of {n} runs')
    # config 1: ONE rollout, 200 steps, 128x128 map (the reference's own CPU-runnable case)
    cfg1, _, pts1, masks1, z1, mu1, ctrl1 = build_problem(1, 200, N, None, integ, seed=0, grid_res=0.1)
    spec1 = _oracle_spec(cfg1, pts1, masks1, integ, 0.1)

    def c1():
        with torch.no_grad():
            orc.rollout(spec1, z1.unsqueeze(0), ctrl1, friction=mu1.unsqueeze(0))
    cores = _best_threads(c1, cand)
    torch.set_num_threads(cores)
    t, n = _time_cpu(c1, 4.0, max_runs=8)
    torch.set_num_threads(all_threads)
    legs['c1_forward'] = dict(value=200 / t, unit='rollout-steps/s', cores=cores, kind='port',
                              sample=f'B=1 x T=200 x N={N}, 128x128 map (res 0.1), forward no_grad, median of {n} runs')
    same = 'c3_autograd' if WORKLOADS[headline]['backward'] else 'c2_forward'
    head = dict(legs[same])
    head['same_workload_as_headline'] = same
    head['sample'] += f'; {head["cores"]} torch threads = the fastest of {cand} on this host; os.cpu_count()={os.cpu_count()}'
    head['legs'] = legs
    return head


class Runner:
    def __init__(self, args):
        self.args = args
        self.world = int(os.environ.get('WORLD_SIZE', '1'))
        self.rank = int(os.environ.get('RANK', '0'))
        local_rank = int(os.environ.get('LOCAL_RANK', '0'))
        assert torch.cuda.is_available(), 'bench.py needs an MI355X (no CPU fallback)'
        if os.environ.get('MF_BENCH_SINGLE_DEVICE'):      # test rig: all ranks on GPU 0, gloo instead of RCCL
            local_rank = 0
        torch.cuda.set_device(local_rank)
        self.dev = torch.device('cuda', local_rank)
        self.backend = os.environ.get('MF_BENCH_BACKEND', 'nccl')      # "nccl" is RCCL on ROCm
        self.dist_world = 1
        # MF_BENCH_FORCE_DIST=1 with ONE rank: a one-rank process group, every collective of the N > 1 step still issued (RCCL
        # init with device_id, all_reduce(AVG) in place behind a hipGraph replay, the hooked bucket exchange) -- so that code has run
        # on a one-GPU box before the first multi-GPU run
        self.force_dist = bool(os.environ.get('MF_BENCH_FORCE_DIST')) and self.world == 1
        self.dist_on = self.world > 1 or self.force_dist
        if self.dist_on:
            import torch.distributed as dist
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            if self.force_dist:
                from monoforce_amd import dist as mfdist
                os.environ.setdefault('MASTER_PORT', str(_free_port()))
                os.environ.setdefault('RANK', '0')
                os.environ.setdefault('WORLD_SIZE', '1')
                mfdist.FORCE = True
            if self.backend == 'nccl':
                dist.init_process_group('nccl', device_id=self.dev)
            else:
                dist.init_process_group(self.backend)
            self.dist_world = dist.get_world_size()        # what the collective library itself sees
        # PMC-measured HBM bytes per launch (tools/collect_profiles.sh): valid for the library build they were measured on -- the file
        # carries that build's sha256, and a different library gets `traffic: null` with the reason instead of a stale figure
        # (--full only: `roofline` is the one reader)
        traffic_file = os.path.join(REPO, 'profiles', 'hbm_traffic.json')
        self.traffic = json.load(open(traffic_file)) if args.full and os.path.exists(traffic_file) else {}
        self.traffic_stale = None
        want = self.traffic.get('_library_sha256')
        if self.traffic:
            have = library_sha256()
            if want != have:
                self.traffic_stale = (f'profiles/hbm_traffic.json was measured on library build {str(want)[:12]}, this run loads {have[:12]}: '
                                      'regenerate with tools/collect_profiles.sh')
                self.traffic = {}

    def barrier(self):
        if self.dist_on:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(self, v, op='MAX'):
        if self.dist_on:
            import torch.distributed as dist
            tt = torch.tensor([v], device=self.dev if self.backend == 'nccl' else 'cpu', dtype=torch.float64)
            dist.all_reduce(tt, op=getattr(dist.ReduceOp, op))
            v = float(tt.item())
        return v

    def time_exchange(self, fn, n=20):
        """ms per call of the step's gradient exchange ALONE (its collectives and nothing else), max over ranks."""
        rig = self.dist_on and self.backend != 'nccl'      # the one-GPU test rig (gloo on the host's cores: seconds per 55 MB exchange at 8 ranks)
        n = min(n, 2) if rig else n
        for _ in range(1 if rig else 3):
            fn()
        self.barrier()
        t = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize(self.dev)
        return self.max_over_ranks((time.perf_counter() - t) / n * 1e3)

    def run(self, name, steps, warmup, batch=0, events_after=False, measure=True, keep_outputs=False):
        """Time `steps` steps of workload `name` after `warmup` (and the launch-mode calibration).  measure=False (a plain run's
        headline): a bare timed region -- no HIP events in it or after it, no exchange timing, no `roofline`.  keep_outputs: the
        record carries, under `outputs`, host copies of what the LAST timed step handed its caller."""
        from monoforce_amd import _timing
        args, dev, world, rank = self.args, self.dev, self.world, self.rank
        wl = dict(WORKLOADS[name])
        if batch:
            wl['B'] = batch
        if args.points:
            wl['N'] = args.points
        strong = bool(wl.get('strong'))
        B_total = wl['B'] if strong else wl['B'] * world
        B = wl['B'] // world if strong else wl['B']           # rollouts of THIS rank
        assert B >= 1 and (not strong or B * world == wl['B']), f'{wl["B"]} rollouts do not split over {world} ranks'
        T, N = wl['T'], wl['N']
        res = wl.get('grid_res', 0.05)
        # ONE terrain / friction pair, the same on every rank (terrain_seed 0); every rank rolls out its OWN controls (seed = rank)
        cfg, dp, pts, masks, z, mu, ctrl = build_problem(B, T, N, dev, args.integrator, seed=rank, grid_res=res, terrain_seed=0)
        dp.block = args.block
        zd = z.to(dev).unsqueeze(0)       # [1,H,W] map shared by the rollouts + [B,T,2] controls
        md = mu.to(dev).unsqueeze(0)
        cd = ctrl.to(dev)
        if wl.get('encoder'):
            if os.environ.get('MF_MIOPEN_BENCHMARK'):      # let MIOpen time its solvers per convolution shape (first steps slower)
                torch.backends.cudnn.benchmark = True
            from monoforce_amd.terrain_encoder import LiftSplatShoot
            from monoforce_amd.train import EncoderTrainStep, synthetic_encoder_batch
            torch.manual_seed(0)        # identical initial weights on every rank (DDP convention)
            gc = dict(xbound=[-6.4, 6.4, 0.05], ybound=[-6.4, 6.4, 0.05], zbound=[-3.2, 3.2, 6.4], dbound=[0.6, 6.4, 0.1])
            enc = LiftSplatShoot(gc, dict(final_dim=(256, 512))).to(dev).train()
            if os.environ.get('MF_CHANNELS_LAST'):      # A/B (tools/ab_c4_miopen.sh): NHWC weights -> MIOpen's NHWC solvers
                for m_ in enc.modules():      # (conv weights only: the module also holds 4-D non-conv parameters, e.g. the frustum table)
                    if isinstance(m_, torch.nn.Conv2d):
                        m_.weight.data = m_.weight.data.contiguous(memory_format=torch.channels_last)
            ebatch = synthetic_encoder_batch(enc, dp, n_rollouts=B, device=dev, seed=rank)    # the encoder batch is sharded too
            estep = EncoderTrainStep(enc, dp, lr=1e-4, graph=not os.environ.get('MF_BENCH_NO_GRAPH'))
            aug_pool = None
            if wl.get('augment'):      # eight pre-sampled resize + crop augmentations, copied into the batch's tensors before every step
                enc.cache_plan = False
                ga = torch.Generator().manual_seed(1234)
                post_rots, post_trans = ebatch[0][4], ebatch[0][5]
                aug_pool = []
                for _ in range(8):
                    sc = 0.9 + 0.2 * torch.rand(post_rots.shape[:2], generator=ga)
                    pr = torch.eye(3).repeat(*post_rots.shape[:2], 1, 1)
                    pr[..., 0, 0] = sc; pr[..., 1, 1] = sc
                    pt = torch.zeros(post_trans.shape)
                    pt[..., :2] = (torch.rand(*post_trans.shape[:2], 2, generator=ga) - 0.5) * 30.0
                    aug_pool.append((pr.to(dev), pt.to(dev)))
                aug_i = [0]
        elif wl['backward']:
            from monoforce_amd.train import TerrainFitProblem
            from monoforce_amd import synthetic as syn
            z_true = syn.bump_terrain(syn.bump_params(100), 6.4, res).to(dev)       # GT trajectories come from another terrain
            # (graph=True: `prob.step(eager=False)` replays forward + loss + backward as one hipGraph, captured at its first use)
            prob = TerrainFitProblem(dp, z_true, mu.to(dev), cd, graph=True)
            zleaf = z.to(dev).clone().requires_grad_(True)
            mleaf = mu.to(dev).clone().requires_grad_(True)

        use_graph = not os.environ.get('MF_BENCH_NO_GRAPH')
        mode = {'graph': False}
        fwd_graph = fwd_out = None

        def forward_eager():
            with torch.no_grad():
                return dp(zd, cd, friction=md)

        def step():
            eager = _timing.sampled() or not mode['graph']       # steps bracketed with HIP events run launch by launch
            if wl.get('encoder'):
                if aug_pool is not None:      # the data loader's part: this step's augmentation, in place (two small copies)
                    pr, pt = aug_pool[aug_i[0] % len(aug_pool)]
                    aug_i[0] += 1
                    ebatch[0][4].copy_(pr); ebatch[0][5].copy_(pt)
                return estep.step(ebatch, eager=eager)
            if wl['backward']:
                return prob.step(zleaf, mleaf, eager=eager)
            if eager:
                return forward_eager()
            fwd_graph.replay()
            return fwd_out      # (the graph's own output tensors, rewritten by every replay)

        for _ in range(warmup):
            step()
        launch = None
        if use_graph:
            # Launch mode of the timed region, chosen by measurement on THIS host (untimed, after the warm-up): the step replayed
            # as one hipGraph (~20 us of host work, but every graph node pays a few us more on the device) against the step
            # launched call by call (0.15 ms of Python and launch calls forward, 0.3 ms forward + backward: faster while the host
            # keeps ahead of the kernels, host-bound on a loaded or slower box and at the small configs).  Same kernels, same
            # work either way.
            if not wl['backward'] and not wl.get('encoder'):
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    forward_eager()
                torch.cuda.current_stream(dev).wait_stream(side)
                from monoforce_amd.capture import capture
                fwd_graph = torch.cuda.CUDAGraph()
                with capture(fwd_graph, stream=side, capture_error_mode='thread_local'):
                    fwd_out = forward_eager()

            def timed(graph, n=(2 if (self.dist_on and self.backend != 'nccl') else 8) if wl.get('encoder') else 32):      # (gloo test rig: every encoder step carries a host-side exchange)
                mode['graph'] = graph
                step()
                torch.cuda.synchronize(dev)
                t = time.perf_counter()
                for _ in range(n):
                    step()
                torch.cuda.synchronize(dev)
                return (time.perf_counter() - t) / n * 1e3
            if wl.get('encoder') and self.dist_on and self.backend != 'nccl':      # test rig: no calibration of the launch mode (six more exchanges)
                t_graph, t_eager = 0.0, float('inf')
            else:
                t_graph, t_eager = self.max_over_ranks(timed(True)), self.max_over_ranks(timed(False))
            mode['graph'] = t_graph < 1.03 * t_eager       # near a tie the replay wins: its timed region does not depend on the host keeping ahead
            split = bool(wl.get('encoder')) and self.dist_on      # collectives are not captured: two graphs around the live exchange
            launch = {'mode': ('two hipGraph replays around the exchange' if split else 'one hipGraph replay per step') if mode['graph'] else 'launch by launch',
                      'calibration_ms_per_step': None if t_eager == float('inf') else {'graph': t_graph, 'eager': t_eager}}
        self.barrier()
        # HIP events around the C-ABI launches of every 32nd step of the timed region, on the stream the kernel is launched on
        # (around all of them they cost 33 us of a 0.55 ms step: each record is a packet of its own between two kernels)
        # (`events_after`, the side workloads of the default line -- a handful of steps each: a step bracketed with events runs launch by
        #  launch, and one such step among five replays of a 16 ms graph IS the average on a host that is slow at launching -- c4 read
        #  20.1 ms where its replays take 16.4.  Their timed region is K replays; the kernel durations come from sampled steps after it.)
        if measure and not events_after:
            _timing.start(every=EVENT_EVERY)
        t0 = time.perf_counter()
        for _ in range(steps):
            _timing.next_step()
            last = step()
        self.barrier()
        elapsed = time.perf_counter() - t0
        outputs = None
        if keep_outputs:      # (before anything else runs a step: the encoder's steps update its weights)
            if wl.get('encoder'):
                loss, (l_geom, l_terr, l_phys) = last
                named = {'loss': loss, 'loss_geom': l_geom, 'loss_terrain': l_terr, 'loss_phys': l_phys}
            elif wl['backward']:      # the loss, and the gradients the step leaves in .grad of the terrain and friction leaves
                named = {'loss': last, 'grad_z': zleaf.grad, 'grad_mu': mleaf.grad}
            else:
                (Xs, Xds, Rs, Om), (Fs, Ff) = last
                named = {'Xs': Xs, 'Xds': Xds, 'Rs': Rs, 'Om': Om, 'Fs': Fs, 'Ff': Ff}
            outputs = {k: (v.detach() if v.dtype in (torch.float32, torch.float64) else v.detach().double()).cpu().numpy()
                       for k, v in named.items() if v is not None}
        mode_text = 'encoder train step (fwd+bwd+Adam)' if wl.get('encoder') else 'forward+backward' if wl['backward'] else 'forward'
        integ = 'odeint-euler (reference default)' if args.integrator == 1 else 'dynamics()'
        H = int(round(12.8 / res))
        if not measure:
            elapsed_min, elapsed = self.max_over_ranks(elapsed, 'MIN'), self.max_over_ranks(elapsed)
            del dp
            return self._record(name, wl, steps, warmup, elapsed, elapsed_min, strong, B, B_total, T, N, H, res, integ, mode_text, launch, {},
                                outputs), (N, T)
        # more samples of the kernel durations from steps run right after the region (untimed; a bracketed step runs launch by launch,
        # which is why the region itself carries few of them: at K = 20 every 8th step was 3 of 20 steps at 0.45-0.58 instead of 0.385 ms)
        if events_after:
            _timing.start(every=1)
        else:
            _timing.set_every(1)
        for _ in range(max(2, min(steps // 2, 6)) if events_after else 4):
            _timing.next_step()
            step()
        self.barrier()
        kern = {k: float(np.mean(v)) for k, v in _timing.stop().items()}       # average launch duration per kernel, ms
        kernels_run = _timing.launches()      # which kernel template the library's dispatcher picked (mf_last_launch), per sampled launch
        elapsed_min, elapsed = self.max_over_ranks(elapsed, 'MIN'), self.max_over_ranks(elapsed)
        # the exchange step on its own (the backward's one collective), so that a scaling curve can be read
        comm_ms = None
        if self.dist_on and wl['backward']:
            if wl.get('encoder'):
                comm_ms = self.time_exchange(estep.exchange_only, n=5)
            else:
                zero = torch.zeros((), device=dev)
                comm_ms = self.time_exchange(lambda: prob._exchange(zleaf, mleaf, zero))

        P4 = 4 * 59 * 16 * 32                                  # frustum points per sample at the config-4 shapes
        # the forward of a fit / train step writes no forces (states only; c3f and c2 write all six outputs)
        states_only = bool(wl['backward'])      # (TerrainFitProblem / EncoderTrainStep run DPhysics.physics_loss_rollout: Fs = Ff = NULL)
        fwd_alg = (fwd_states_only_bytes_per_rollout_step(N) if states_only else fwd_bytes_per_rollout_step(N)) * B * T
        hbm = {'rollout_fwd_kernel': fwd_hbm_bytes_per_rollout_step(N, forces=not states_only) * B * T,
               'rollout_bwd_kernel': bwd_hbm_bytes_per_rollout_step(N) * B * T}
        alg = {'rollout_fwd_kernel': fwd_alg, 'rollout_bwd_kernel': bwd_bytes_per_rollout_step(N) * B * T,
               'splat_fwd_kernel': 4 * 64 * P4 + 12 * P4 + 4 * 64 * 256 * 256, 'splat_bwd_kernel': 4 * 64 * 256 * 256 + 4 * 64 * P4,
               'splat_prepare': 20 * P4,
               # lift fused into the splat: depth 4 P + context 4*64*pixels + out / the reverse + the voxel-major rows
               'lift_splat_fwd_kernel': 4 * P4 + 4 * 64 * (P4 // 59) + 4 * 64 * 256 * 256,
               'lift_splat_bwd_kernel': 4 * 64 * 256 * 256 + 8 * P4 + 2 * 4 * 64 * (P4 // 59),
               'physics_loss_fwd': 12 * 50 * B * 2, 'physics_loss_bwd': 12 * 50 * B * 2}
        kern = {k: v for k, v in kern.items() if k in alg}
        dom = max(kern, key=kern.get)                          # the dominant hand-written kernel of the step
        per_kernel = {k: {'ms': v, 'algorithmic_bytes': alg[k], 'GB/s': alg[k] / (v * 1e-3) / 1e9,
                          'frac': alg[k] / (v * 1e-3) / 1e9 / HBM_PEAK_GBS,
                          # the bytes of the model that must cross HBM (no cache-served map cells / scatter RMW); splat: all of them
                          'hbm_bytes_model': hbm.get(k, alg[k]), 'frac_hbm': hbm.get(k, alg[k]) / (v * 1e-3) / 1e9 / HBM_PEAK_GBS}
                      for k, v in kern.items()}
        for k in ('rollout_fwd_kernel', 'rollout_bwd_kernel'):      # what THIS instantiation is asked to move, beside SURVEY 8d's figure
            if k in per_kernel:
                mb, terms, _ = instance_bytes_per_rollout_step(kernels_run.get(k), N, T=T)
                per_kernel[k].update({'instance': kernels_run.get(k), 'model_bytes_per_rollout_step': mb, 'model_terms': terms,
                                      'frac_model': (mb * B * T / (kern[k] * 1e-3) / 1e9 / HBM_PEAK_GBS) if mb else None,
                                      'regime': regime_of(kernels_run.get(k), B, N)})
                tr = self.traffic.get(name if not batch else f'{name}_B{B}', {}).get(k)
                per_kernel[k]['traffic'] = tr
                per_kernel[k]['frac_traffic'] = (tr / (kern[k] * 1e-3) / 1e9 / HBM_PEAK_GBS) if tr else None
        if 'rollout_fwd_kernel' in per_kernel:
            per_kernel['rollout_fwd_kernel']['bytes_model'] = (
                f'states only (no force rows): controls 8 + states 72 + map cells 32 N = {fwd_states_only_bytes_per_rollout_step(N)} B per rollout-step'
                if states_only else f'all six outputs: 80 + 56 N = {fwd_bytes_per_rollout_step(N)} B per rollout-step')
        if 'rollout_bwd_kernel' in per_kernel:
            per_kernel['rollout_bwd_kernel']['bytes_model'] = (
                f'SURVEY 8d: 160 + 120 N = {bwd_bytes_per_rollout_step(N)} B per rollout-step (of which 72 + 24 N are upstream-gradient rows a fused '
                f'physics loss never reads: the kernel forms dL/dXs itself)')
        achieved = per_kernel[dom]['GB/s']
        traffic = self.traffic.get(name if not batch else f'{name}_B{B}', {}).get(dom)
        # the per-step record small default-integrator launches keep in the forward for the backward (MfRolloutFwdBufs.rec): real
        # bytes on top of the algorithmic ones -- a recompute-for-storage trade, reported so that `traffic` reads right
        rec_bytes = 0
        if wl['backward'] and not wl.get('encoder'):
            import ctypes as C
            from monoforce_amd import _lib
            d = _lib.MfRolloutDesc(B=B, T=T, N=N, H=int(round(12.8 / res)), W=int(round(12.8 / res)), integrator=args.integrator,
                                   math_mode=_lib.MF_MATH_FAST, force_stride=max(N, 4), map_shared=1, layout=_lib.MF_LAYOUT_TIME_MAJOR)
            rec_bytes = int(_lib.lib().mf_rollout_record_bytes(C.byref(d)))
        out = {
            **self._record(name, wl, steps, warmup, elapsed, elapsed_min, strong, B, B_total, T, N, H, res, integ, mode_text, launch,
                           kernels_run, outputs),
            'comm_ms': comm_ms,
            'roofline': {'bound': 'hbm', 'achieved': achieved, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': achieved / HBM_PEAK_GBS,
                         'traffic': traffic,
                         # the PMC-measured HBM bytes per launch over the kernel's measured duration: what the memory system really sustained
                         'frac_traffic': (traffic / (kern[dom] * 1e-3) / 1e9 / HBM_PEAK_GBS) if traffic else None,
                         **({'record_bytes_per_launch': rec_bytes,
                             'traffic_note': 'traffic includes the per-step record the forward writes and the backward reads instead of '
                                             'recomputing it (record_bytes_per_launch; DESIGN.md 4.2b) -- not re-reads'} if rec_bytes else {}),
                         'traffic_source': ('profiles/hbm_traffic.json (rocprofv3 PMC passes of this command on THIS library build -- sha256 checked; '
                                            'not re-measured in this run)' if traffic else self.traffic_stale),
                         'frac_hbm': per_kernel[dom]['frac_hbm'], 'hbm_bytes_model_per_launch': per_kernel[dom]['hbm_bytes_model'],
                         'frac_model': per_kernel[dom].get('frac_model'), 'model_bytes_per_rollout_step': per_kernel[dom].get('model_bytes_per_rollout_step'),
                         'model_terms': per_kernel[dom].get('model_terms'), 'regime': per_kernel[dom].get('regime'),
                         'frac_note': '`frac` = SURVEY 8d algorithmic bytes (the contract figure: map cells counted even when cache-served, upstream rows '
                                      'counted even when the instantiation never reads them) / kernel time / 8 TB/s; `frac_model` = the bytes THIS '
                                      'instantiation is asked to move (model_terms); `frac_hbm` = SURVEY 8d without the cache-served bytes; `traffic` / '
                                      '`frac_traffic` = HBM bytes at the PMC counters -- the only one of the four that is HBM bandwidth',
                         'kernel': dom, 'kernel_ms': kern[dom], 'kernel_ms_from': ('HIP events around the launches of sampled steps run right after the timed region (the region itself: replays only)'
                                                           if events_after else f'HIP events around the launches of every {EVENT_EVERY}th timed step and of four steps run right after the region'),
                         'algorithmic_bytes_per_launch': alg[dom], 'bytes_per_rollout_step': alg[dom] // (B * T),
                         'per_kernel': per_kernel},
        }
        del dp
        return out, (N, T)

    def _record(self, name, wl, steps, warmup, elapsed, elapsed_min, strong, B, B_total, T, N, H, res, integ, mode, launch, kernels_run,
                outputs):
        """The headline part of a workload's record: rate, ms per step, scaling, config (`elapsed`: the max over the ranks)."""
        out = {
            'value': B_total * T * steps / elapsed, 'steps': steps, 'warmup': warmup, 'ms_per_step': elapsed / steps * 1e3,
            'ms_per_step_ranks': {'min': elapsed_min / steps * 1e3, 'max': elapsed / steps * 1e3},
            'comm_ms': None, 'scaling': 'strong' if strong else 'weak',
            'config': {'workload': f'{name}: B={B}/GPU x T={T} x N={N} contact points, {H}x{H} grid (res {res} m), one shared '
                                   f'terrain+friction map (the same on every rank), integrator={integ}, {mode}; {wl["desc"]}',
                       'rollouts_per_gpu': B, 'rollouts_total': B_total, 'horizon': T, 'contact_points': N, 'grid': [H, H],
                       'parallelism': f'rollout-sharded x{self.world}',
                       'launch': {**(launch or {'mode': 'launch by launch'}), 'kernels': kernels_run}},
        }
        if outputs is not None:
            out['outputs'] = outputs
        return out

    def batch_sweep(self, N, T, batches=(256, 1024, 4096, 8192, 16384, 32768, 65536), private_batches=(256, 1024)):
        """Forward and backward rollout kernels over the batch (256 ... 65 536 rollouts; kernel time from HIP events; not part
        of `value`), one shared map pair; and the per-rollout-map variant (`per_rollout_maps`: one 256 x 256 height + friction pair PER
        rollout -- 512 KiB each, so 1024 rollouts hold 512 MB of maps and as much again of map gradients; beyond that the variant is
        memory for its own sake and is not swept)."""
        from monoforce_amd import _timing
        from monoforce_amd.train import TerrainFitProblem
        from monoforce_amd import synthetic as syn
        dev = self.dev
        sweep, private = {}, {}

        def row(Bs, f_ms, b_ms, launches, step_ms=None):
            fg = fwd_bytes_per_rollout_step(N) * Bs * T / (f_ms * 1e-3) / 1e9
            bg = bwd_bytes_per_rollout_step(N) * Bs * T / (b_ms * 1e-3) / 1e9
            out = {'fwd_ms': f_ms, 'fwd_frac': fg / HBM_PEAK_GBS, 'fwd_rollout_steps_per_s': Bs * T / (f_ms * 1e-3),
                   'fwd_frac_hbm': fwd_hbm_bytes_per_rollout_step(N) * Bs * T / (f_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                   'bwd_ms': b_ms, 'bwd_frac': bg / HBM_PEAK_GBS, 'bwd_rollout_steps_per_s': Bs * T / (b_ms * 1e-3),
                   'bwd_frac_hbm': bwd_hbm_bytes_per_rollout_step(N) * Bs * T / (b_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 'kernels': launches}
            # three fractions per leg: SURVEY 8d's figure (`*_frac`), the bytes the instantiation that RAN is asked to
            # move (`*_frac_model`), and HBM bytes at the PMC counters where a pass is on file (`*_frac_traffic`, profiles/hbm_traffic.json)
            for leg, ms in (('fwd', f_ms), ('bwd', b_ms)):
                inst = launches.get(f'rollout_{leg}_kernel')
                mb, terms, _ = instance_bytes_per_rollout_step(inst, N, T=T)
                tr = self.traffic.get(f'c3_B{Bs}', {}).get(f'rollout_{leg}_kernel') if leg == 'bwd' else self.traffic.get(f'c3f_B{Bs}', {}).get('rollout_fwd_kernel')
                out.update({f'{leg}_model_bytes_per_rollout_step': mb, f'{leg}_model_terms': terms,
                            f'{leg}_frac_model': (mb * Bs * T / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if mb else None,
                            f'{leg}_traffic': tr, f'{leg}_frac_traffic': (tr / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if tr else None,
                            f'{leg}_bound': regime_of(inst, Bs, N)})
                if out[f'{leg}_frac'] > 0.79 or (out[f'{leg}_frac_model'] or 0) > 0.79:      # beyond what HBM can deliver (~6.3 of 8 TB/s): not HBM bandwidth
                    out[f'{leg}_note'] = ('cache-served: a model fraction above 0.79 exceeds what HBM delivers -- the gathered cells and the '
                                          'cell-gradient read-modify-writes of the model stay in L2 / LDS; read `frac_traffic` / `frac_hbm` for HBM')
            if step_ms is not None:
                out['step_ms'] = step_ms      # forward + loss + backward + gradient reduction of one fit step, HIP events around the step
            return out

        for Bs in batches:
            _, dps, _, _, z, mu, cs = build_problem(Bs, T, N, dev, self.args.integrator, seed=0)
            cs = cs.to(dev)
            prob = TerrainFitProblem(dps, syn.bump_terrain(syn.bump_params(100), 6.4, 0.05).to(dev), mu.to(dev), cs, graph=not os.environ.get('MF_BENCH_NO_GRAPH'))
            zl, ml = z.to(dev).clone().requires_grad_(True), mu.to(dev).clone().requires_grad_(True)
            zd, md = z.to(dev).unsqueeze(0), mu.to(dev).unsqueeze(0)
            for _ in range(2):
                prob.step(zl, ml, eager=True)
            _timing.start()
            for _ in range(3):
                prob.step(zl, ml, eager=True)
            launches = {'rollout_bwd_kernel': _timing.launches().get('rollout_bwd_kernel')}
            k = _timing.stop()
            # the whole fit step (forward + loss + backward + reduction of the gradient copies), replayed as one hipGraph: HIP events around 6 steps
            prob.step(zl, ml)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(6):
                prob.step(zl, ml)
            e1.record()
            torch.cuda.synchronize(dev)
            step_ms = e0.elapsed_time(e1) / 6
            launches['step'] = {kk: float(np.mean(v)) for kk, v in k.items()}      # every hand-written launch of the step, ms
            with torch.no_grad():       # the plain forward (all six outputs, no saved rows for a backward)
                dps(zd, cs, friction=md)
                _timing.start()
                for _ in range(3):
                    dps(zd, cs, friction=md)
                launches['rollout_fwd_kernel'] = _timing.launches().get('rollout_fwd_kernel')
                kf = _timing.stop()
            sweep[str(Bs)] = row(Bs, float(np.mean(kf['rollout_fwd_kernel'])), float(np.mean(k['rollout_bwd_kernel'])), launches, step_ms=step_ms)
            del dps, prob, cs, zl, ml
            torch.cuda.empty_cache()      # return the sweep's multi-GB blocks now, not inside a later workload's timed region
        for Bs in private_batches:      # one map pair PER ROLLOUT: [B,H,W] leaves, the loss on every 10th pose (the rows physics_loss stamps)
            _, dps, _, _, z, mu, cs = build_problem(Bs, T, N, dev, self.args.integrator, seed=0)
            cs = cs.to(dev)
            zb = z.to(dev).unsqueeze(0).repeat(Bs, 1, 1).requires_grad_(True)
            mb = mu.to(dev).unsqueeze(0).repeat(Bs, 1, 1).requires_grad_(True)

            def fb():
                zb.grad = mb.grad = None
                (Xs, _, _, _), _ = dps(zb, cs, friction=mb)
                (Xs[:, 9::10] ** 2).mean().backward()
            for _ in range(2):
                fb()
            _timing.start()
            for _ in range(3):
                fb()
            launches = _timing.launches()
            k = _timing.stop()
            private[str(Bs)] = row(Bs, float(np.mean(k['rollout_fwd_kernel'])), float(np.mean(k['rollout_bwd_kernel'])), launches)
            private[str(Bs)]['note'] = ('forward = the autograd forward of this route (all six outputs + the rows kept for the backward); backward reads '
                                        'dL/dXs rows and writes [B,H,W] gradients of both maps')
            del dps, cs, zb, mb
            torch.cuda.empty_cache()
        first = {kind or 'survey_8d': {leg: next((int(b) for b in sweep if (sweep[b].get(f'{leg}_frac{kind}') or 0) >= 0.4), None) for leg in ('fwd', 'bwd')}
                 for kind in ('', '_model', '_hbm', '_traffic')}
        return {'batches': sweep, 'per_rollout_maps': private, 'first_B_at_40pct': first,
                'first_B_at_40pct_note': 'per fraction: survey_8d = SURVEY 8d bytes; _model = the instantiation\'s own bytes; _hbm = SURVEY 8d without '
                                         'cache-served bytes; _traffic = PMC-measured HBM bytes (None: no batch with a PMC pass reaches 40 % of HBM)'}


def points_sweep(r, T, integ, points=(32, 175, 223), batches=(64, 1024, 4096)):
    """SURVEY 8d's secondary sweep -- N in {32, 175 (tradr), 223 (marv, the reference notebook's body)} -- over the batch, so that the reference's
    body sizes have a saturation curve and not only the B = 64 latency point: the fit step's states-only forward and its
    backward, kernel times from HIP events, SURVEY 8d's bytes and the instantiation's own."""
    from monoforce_amd import _timing
    from monoforce_amd.train import TerrainFitProblem
    from monoforce_amd import synthetic as syn
    dev, rows = r.dev, {}
    for Np in points:
        for Bs in batches:
            _, dps, _, _, z, mu, cs = build_problem(Bs, T, Np, dev, integ, seed=0)
            cs = cs.to(dev)
            prob = TerrainFitProblem(dps, syn.bump_terrain(syn.bump_params(100), 6.4, 0.05).to(dev), mu.to(dev), cs)
            zl, ml = z.to(dev).clone().requires_grad_(True), mu.to(dev).clone().requires_grad_(True)
            prob.step(zl, ml)
            _timing.start()
            for _ in range(2):
                prob.step(zl, ml)
            inst = _timing.launches()
            k = {a: float(np.mean(v)) for a, v in _timing.stop().items()}
            f_ms, b_ms = k['rollout_fwd_kernel'], k['rollout_bwd_kernel']
            row = {'fwd_ms': f_ms, 'bwd_ms': b_ms, 'kernels': {a: inst.get(a) for a in ('rollout_fwd_kernel', 'rollout_bwd_kernel')},
                   'fwd_rollout_steps_per_s': Bs * T / (f_ms * 1e-3), 'bwd_rollout_steps_per_s': Bs * T / (b_ms * 1e-3),
                   'fwd_frac': fwd_states_only_bytes_per_rollout_step(Np) * Bs * T / (f_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                   'bwd_frac': bwd_bytes_per_rollout_step(Np) * Bs * T / (b_ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
            for leg, ms in (('fwd', f_ms), ('bwd', b_ms)):
                mb, _, _ = instance_bytes_per_rollout_step(inst.get(f'rollout_{leg}_kernel'), Np, T=T)
                row[f'{leg}_frac_model'] = (mb * Bs * T / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if mb else None
            rows[f'N{Np}_B{Bs}'] = row
            del dps, prob, cs, zl, ml
            torch.cuda.empty_cache()
    return {'rows': rows, 'bytes_model': 'fwd_frac: states-only forward 80 + 32 N B per rollout-step; bwd_frac: SURVEY 8d 160 + 120 N; *_frac_model: the '
                                           'instantiation that ran (positions-only upstream, 16-byte record)'}


def api_workload(r, T, N, integ, B=1024, iters=24):
    """`c3_api`: the DROP-IN route a user of the unchanged scripts gets (scripts/fit_terrain.py:53-62, scripts/train.py:399-406): `DPhysics.forward`
    (six outputs), `monoforce.losses.physics_loss` on the returned states, `loss.backward()`.  Timed twice: as it runs by default -- after three
    identical cycles the module replays the whole step as ONE hipGraph (monoforce_amd/api_cache.py: rollout with force rows + the loss inside
    the launches + backward; `physics_loss` returns the graph's loss, its backward hands out the graph's gradients) -- and launch by launch
    (MF_API_GRAPH=0: forward kernel, mf_nearest_steps + mf_physics_loss_value / _bwd, backward kernel reading dense dL/dXs rows), with the
    host time of each of the three calls."""
    from monoforce_amd import _timing, api_cache
    from monoforce.losses import physics_loss      # the reference's import path (the shim re-exports monoforce_amd.losses)
    from monoforce_amd import synthetic as syn
    dev = r.dev
    out = {}
    for mode in ('cached', 'launch_by_launch'):
        keep, api_cache.ENABLED = api_cache.ENABLED, mode == 'cached'
        try:
            cfg, dp, _, _, z, mu, ctrl = build_problem(B, T, N, dev, integ, seed=0)
            cd = ctrl.to(dev)
            with torch.no_grad():
                (Xg, Xdg, Rg, Og), _ = dp(syn.bump_terrain(syn.bump_params(100), 6.4, 0.05).to(dev).unsqueeze(0), cd, friction=mu.to(dev).unsqueeze(0))
            full_ts = torch.linspace(0, cfg.traj_sim_time, int(cfg.traj_sim_time / cfg.dt), device=dev)[:T]
            sel = torch.arange(9, T, 10, device=dev)                      # 10 Hz ground-truth poses (datasets/rough.py:217,238)
            pred_ts, gt_ts = full_ts.unsqueeze(0).expand(B, -1), full_ts[sel].unsqueeze(0).expand(B, -1).contiguous()
            states_gt = [t[:, sel].contiguous() for t in (Xg, Xdg, Rg, Og)]
            zl, ml = z.to(dev).clone().unsqueeze(0).requires_grad_(True), mu.to(dev).clone().unsqueeze(0).requires_grad_(True)
            host = {'forward_call_us': [], 'loss_us': [], 'backward_call_us': []}

            def step(record=False):
                zl.grad = ml.grad = None
                t0 = time.perf_counter()
                states, forces = dp(z_grid=zl, controls=cd, friction=ml)
                t1 = time.perf_counter()
                loss = physics_loss(states_pred=states, states_gt=states_gt, pred_ts=pred_ts, gt_ts=gt_ts, gamma=0.9)
                t2 = time.perf_counter()
                loss.backward()
                t3 = time.perf_counter()
                if record:
                    host['forward_call_us'].append((t1 - t0) * 1e6); host['loss_us'].append((t2 - t1) * 1e6); host['backward_call_us'].append((t3 - t2) * 1e6)
                return loss

            for _ in range(6):      # (the cached step is captured in the fourth call)
                step()
            r.barrier()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(iters):
                step(record=True)
            e1.record()
            torch.cuda.synchronize(dev)
            ms = (time.perf_counter() - t0) / iters * 1e3
            row = {'ms_per_step': ms, 'device_ms_per_step': e0.elapsed_time(e1) / iters, 'host_us_per_call': {k: float(np.median(v)) for k, v in host.items()},
                   'replays': getattr(dp.__dict__.get('_api_step_cache'), 'replays', 0)}
            if mode == 'launch_by_launch':
                _timing.start()
                for _ in range(4):
                    _timing.next_step()
                    step()
                row['kernels'] = _timing.launches()
                kern = {k: float(np.mean(v)) for k, v in _timing.stop().items()}
                alg = {'rollout_fwd_kernel': fwd_bytes_per_rollout_step(N) * B * T, 'rollout_bwd_kernel': bwd_bytes_per_rollout_step(N) * B * T}
                row['per_kernel'] = {k: {'ms': v, 'algorithmic_bytes': alg[k], 'frac': alg[k] / (v * 1e-3) / 1e9 / HBM_PEAK_GBS} for k, v in kern.items() if k in alg}
                row['kernel_ms_sum'] = float(sum(kern.values()))
            out[mode] = row
            del dp
        finally:
            api_cache.ENABLED = keep
    ms = out['cached']['ms_per_step']
    return {'value': B * T / (ms * 1e-3), 'unit': 'rollout-steps/s', 'ms_per_step': ms,
            'workload': f'c3_api: B={B} x T={T} x N={N}, one shared 256x256 map pair, DPhysics.forward (six outputs) + monoforce.losses.physics_loss (50 stamps) + '
                        f'loss.backward() as the reference\'s scripts write them; default behaviour: the step replayed as one hipGraph after three identical cycles',
            'launch': {'mode': 'one hipGraph replay per step (api_cache)' if out['cached']['replays'] >= iters else 'launch by launch'},
            'cached': out['cached'], 'launch_by_launch': out['launch_by_launch'],
            'per_kernel': out['launch_by_launch'].get('per_kernel', {})}


def shoot_workload(r, T, N, integ, B=16384, iters=8):
    """Sampling-based planning (monoforce_node.py:41-126): B control samples, one shared map, force path cost, argmin."""
    from monoforce_amd import _timing
    from monoforce_amd.planner import TrajectoryShooter, sample_controls
    dev = r.dev
    cfg, dp, _, _, z, mu, _ = build_problem(B, T, N, dev, integ, seed=0)
    zd, md = z.to(dev), mu.to(dev)
    c = sample_controls(B, cfg, dev, torch.Generator(device=dev).manual_seed(0))
    sh = TrajectoryShooter(dp, n_trajs=B, cost='force')
    for _ in range(3):
        sh.shoot(zd, friction=md, controls=c)
    torch.cuda.synchronize(dev)
    _timing.start()
    t0 = time.perf_counter()
    for _ in range(iters):
        sh.shoot(zd, friction=md, controls=c)        # int(argmin) inside synchronises every iteration, like the node
    torch.cuda.synchronize(dev)
    ms = (time.perf_counter() - t0) / iters * 1e3
    kms = float(np.mean(_timing.stop()['rollout_fwd_kernel']))
    return {'value': B * T / (ms * 1e-3), 'unit': 'rollout-steps/s', 'ms_per_step': ms,
            'workload': f'shoot: {B} sampled control sequences x T={T} x N={N}, one shared map, path-cost kernel + force cost + argmin',
            'per_kernel': {'rollout_fwd_kernel': {'ms': kms, 'bytes_per_rollout_step': 8 + 16 + 32 * N,
                                                  'GB/s': (8 + 16 + 32 * N) * B * T / (kms * 1e-3) / 1e9}}}


COMPACT_LIMIT = 4096        # bytes: the driver parses the LAST stdout line and holds only a few KB of it (BENCH_r05: a 28.8 KB line was unparseable)


def _short(text, n):
    text = str(text)
    return text if len(text) <= n else text[:n - 3] + '...'


def _r(v, sig=6):
    """Round floats to `sig` significant digits (the compact line only; the detail file keeps every digit)."""
    if isinstance(v, float) and v == v and v not in (float('inf'), float('-inf')) and v != 0.0:
        return float(f'%.{sig}g' % v)
    return v


def compact_line(out, detail_file=None):
    """The ONE result line, the last on stdout: the contract's keys + `roofline` + `cpu_baseline` (the last two: --full), every value a
    number or a short string.  Sweeps, side workloads, per-kernel tables, kernel-name strings and CPU legs live in the detail file (`detail`)."""
    cfg, roof = out['config'], out.get('roofline') or {}
    c = {k: _r(out.get(k)) for k in ('metric', 'value', 'unit', 'n_gpus', 'world_size', 'backend', 'steps', 'warmup', 'ms_per_step')}
    if out.get('ms_per_step_ranks'):
        c['ms_per_step_ranks'] = {k: _r(v) for k, v in out['ms_per_step_ranks'].items()}
    c['comm_ms'] = _r(out.get('comm_ms'))
    c.update({k: out.get(k) for k in ('higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data')})
    c['config'] = {'workload': _short(cfg['workload'], 200),
                   **{k: cfg.get(k) for k in ('rollouts_per_gpu', 'rollouts_total', 'horizon', 'contact_points', 'grid', 'parallelism')},
                   'launch': {'mode': (cfg.get('launch') or {}).get('mode')}}
    c['roofline'] = {k: _r(roof.get(k)) for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'frac_traffic', 'frac_hbm', 'frac_model', 'kernel', 'kernel_ms',
                                                  'algorithmic_bytes_per_launch', 'bytes_per_rollout_step', 'model_bytes_per_rollout_step',
                                                  'record_bytes_per_launch')
                     if k in roof}
    c['roofline']['kernel_instance'] = _short(((cfg.get('launch') or {}).get('kernels') or {}).get(roof.get('kernel'), ''), 120)
    if roof.get('regime'):
        c['roofline']['regime'] = _short(roof['regime'], 160)
    pk = roof.get('per_kernel') or {}
    c['roofline']['per_kernel_ms'] = {k: _r(v['ms'], 4) for k, v in pk.items() if isinstance(v, dict) and 'ms' in v and not k.endswith('_all_outputs')}
    if 'roofline' not in out:      # a plain run: no roofline measured
        del c['roofline']
    if out.get('forward_only'):
        f = out['forward_only']
        c['forward_only'] = {'value': _r(f['value']), 'ms_per_step': _r(f['ms_per_step']), 'kernel_ms': _r(f['roofline'].get('kernel_ms')),
                             'frac': _r(f['roofline'].get('frac'))}
    if 'cpu_baseline' in out:
        cb = out['cpu_baseline']
        c['cpu_baseline'] = None if cb is None else {**{k: _r(cb.get(k)) for k in ('value', 'unit', 'cores', 'kind')},
                                                    'sample': _short(cb.get('sample', ''), 420)}
    ow = out.get('other_workloads') or {}
    if ow:      # one number per side workload; everything else about them is in the detail file
        c['other_ms_per_step'] = {k: _r(v.get('ms_per_step'), 4) for k, v in ow.items()}
    c['detail'] = detail_file
    line = json.dumps(c, separators=(',', ':'))
    if len(line) >= COMPACT_LIMIT:      # never let an over-long string cost the round its measurement again
        for k in ('other_ms_per_step', 'forward_only'):
            c.pop(k, None)
        c.get('roofline', {}).pop('per_kernel_ms', None)
        c['config']['workload'] = _short(c['config']['workload'], 80)
        if c.get('cpu_baseline'):
            c['cpu_baseline']['sample'] = _short(c['cpu_baseline']['sample'], 120)
        line = json.dumps(c, separators=(',', ':'))
    assert len(line) < COMPACT_LIMIT, len(line)
    return line


def library_sha256():
    import hashlib
    from monoforce_amd import _lib
    path = getattr(_lib, 'LIB_PATH', None) or os.path.join(REPO, 'monoforce_amd', 'csrc', 'libmonoforce_hip.so')
    h = hashlib.sha256()
    with open(path, 'rb') as f:
        for chunk in iter(lambda: f.read(1 << 20), b''):
            h.update(chunk)
    return h.hexdigest()


DUMP_LIMIT = 60 * 10 ** 6      # bytes of array data --dump-outputs writes at most: 64 MB with room for the .npy headers
DUMP_SEED = 0


def dump_outputs(arrays, out_dir, limit=DUMP_LIMIT, seed=DUMP_SEED):
    """Write {name: float32 / float64 array} as out_dir/<name>.npy.  Over `limit` bytes in all, the arrays whose leading dimension
    is the largest one (the rollouts) keep the same rows: a sorted sample drawn with a fixed seed, as many as fit -- the same rows
    in every run with the same arguments, whichever build of the project runs."""
    os.makedirs(out_dir, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    lead = max((a.shape[0] for a in arrays.values() if a.ndim >= 2), default=0)
    rows = None
    if total > limit and lead:
        big = sum(a.nbytes for a in arrays.values() if a.ndim >= 2 and a.shape[0] == lead)
        k = int((limit - (total - big)) // (big // lead))
        assert k >= 1, 'the outputs do not fit the dump limit even at one row each'
        rows = np.sort(np.random.default_rng(seed).choice(lead, size=k, replace=False))
    written = 0
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        if rows is not None and a.ndim >= 2 and a.shape[0] == lead:
            a = np.ascontiguousarray(a[rows])
        np.save(os.path.join(out_dir, f'{name}.npy'), a)
        written += a.nbytes
    assert written <= limit, written
    sampled = f'; rows sampled: {len(rows)} of {lead} (seed {seed})' if rows is not None else ''
    print(f'bench.py: wrote {len(arrays)} output arrays ({written / 2**20:.1f} MiB) to {out_dir}{sampled}', file=sys.stderr)
    return rows


def _free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def spawn_ranks(n):
    """`--gpus n` without a launcher: re-execute this script under torch.distributed.run with n ranks on this node."""
    if not os.environ.get('MF_BENCH_SINGLE_DEVICE'):
        have = torch.cuda.device_count()
        if have < n:
            print(f'bench.py: --gpus {n} but only {have} GPU(s) are visible; refusing to run fewer ranks than asked for', file=sys.stderr)
            return 2
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')       # RCCL / IPC across processes needs dmabuf IPC on this driver
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={n}', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=48)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--workload', default='c3', choices=sorted(WORKLOADS))
    ap.add_argument('--batch', type=int, default=0, help='override rollouts per GPU (total for c5)')
    ap.add_argument('--points', type=int, default=0, help='override contact points')
    ap.add_argument('--integrator', type=int, default=1, help='1 = odeint-euler (reference default), 0 = dynamics()')
    ap.add_argument('--block', type=int, default=0)
    ap.add_argument('--full', action='store_true',
                    help='measure beyond the headline: roofline / per-kernel HIP-event figures, comm_ms, forward_only, sweeps, side workloads, '
                         'cpu_baseline, and write the detail file')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='--full without cpu_baseline')
    ap.add_argument('--no-others', action='store_true', help='--full with the headline workload only (no forward_only / sweep / side workloads)')
    ap.add_argument('--detail', default=os.path.join(REPO, 'bench_detail.json'),
                    help='where rank 0 of a --full run writes the full record (per-kernel tables, batch sweep, side workloads, CPU legs); '
                         'the stdout line stays < 4 KB')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the last timed step computed (rank 0) as DIR/<name>.npy, float32 / float64, at most 64 MB in all')
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')

    world_env = os.environ.get('WORLD_SIZE')
    if args.gpus > 1 and world_env is None:
        sys.exit(spawn_ranks(args.gpus))
    if int(world_env or '1') != args.gpus:
        print(f'bench.py: --gpus {args.gpus} but WORLD_SIZE={world_env}: refusing to run a different number of ranks', file=sys.stderr)
        sys.exit(2)

    r = Runner(args)
    if r.world > 1 and r.dist_world != args.gpus:
        print(f'bench.py: the process group has {r.dist_world} ranks, --gpus {args.gpus}', file=sys.stderr)
        sys.exit(2)
    res, (N, T) = r.run(args.workload, args.steps, args.warmup, batch=args.batch, measure=args.full,
                        keep_outputs=bool(args.dump_outputs) and r.rank == 0)
    outputs = res.pop('outputs', None)
    if outputs is not None:
        dump_outputs(outputs, args.dump_outputs)
    extras, others = {}, {}
    sides = args.full and args.workload == 'c3' and not args.no_others and not args.batch and not args.points
    if sides:
        short = max(args.steps // 3, 5)
        f, _ = r.run('c3f', args.steps, args.warmup)
        extras['forward_only'] = {'value': f['value'], 'unit': 'rollout-steps/s', 'ms_per_step': f['ms_per_step'],
                                  'workload': f['config']['workload'], 'launch': f['config'].get('launch'),
                                  'roofline': {k: f['roofline'][k] for k in ('achieved', 'frac', 'kernel', 'kernel_ms', 'traffic', 'traffic_source')}}
        res['roofline']['per_kernel']['rollout_fwd_kernel_all_outputs'] = f['roofline']['per_kernel']['rollout_fwd_kernel']

        def brief(o):
            return {'value': o['value'], 'unit': 'rollout-steps/s', 'ms_per_step': o['ms_per_step'], 'ms_per_step_ranks': o['ms_per_step_ranks'],
                    'comm_ms': o['comm_ms'], 'scaling': o['scaling'],
                    'workload': o['config']['workload'], 'launch': o['config'].get('launch'), 'per_kernel': o['roofline']['per_kernel']}
        if r.world == 1 and not r.force_dist:
            res['roofline']['batch_sweep'] = r.batch_sweep(N, T)
            res['roofline']['points_sweep'] = points_sweep(r, T, args.integrator)
            for name in ('c1', 'c2', 'ref_nb', 'n32', 'n175'):
                others[name] = brief(r.run(name, short if name in ('c1', 'c2') else 6, 3, events_after=True)[0])
            others['shoot'] = shoot_workload(r, T, N, args.integrator)
            others['c3_api'] = api_workload(r, T, N, args.integrator)
            if args.integrator == 1:      # the other integrator side by side -- dynamics() (use_odeint=False), same shapes
                args.integrator = 0
                try:
                    others['c3_dynamics'] = brief(r.run('c3', short, 3, events_after=True)[0])
                    others['c3f_dynamics'] = brief(r.run('c3f', short, 3, events_after=True)[0])
                finally:
                    args.integrator = 1
            others['c4'] = brief(r.run('c4', 5, 4, events_after=True)[0])
            others['c4_aug'] = brief(r.run('c4_aug', 5, 4, events_after=True)[0])
        else:
            # Several ranks: the headline above is what a scaling run is for; the side workloads must not cost it.  An exception every rank
            # raises alike (a capture the runtime refuses, a shape error) is recorded and the line still goes out; c5 -- the encoder's
            # data-parallel step, the one workload here with a collective INSIDE the step, run so far only over gloo and over ONE RCCL rank
            # (tests/test_c5_gpu.py) -- is part of the default multi-rank run only on request (MF_BENCH_C5=1; `--workload c5` measures it
            # as the headline): a rank-asymmetric failure in it would hang the exchange and with it the line.
            try:
                others['strong_c3'] = brief(r.run('c3', short, 3, batch=max(8192 // r.world, 1), events_after=True)[0])
                others['strong_c3']['scaling'] = 'strong (8192 rollouts in total)'
            except Exception as e:      # noqa: BLE001
                others['strong_c3'] = {'error': f'{type(e).__name__}: {str(e).splitlines()[0][:200]}'}
            if os.environ.get('MF_BENCH_C5'):
                rig = r.backend != 'nccl'      # (the gloo one-GPU test rig: every encoder step carries a host-side exchange of seconds)
                try:
                    others['c5'] = brief(r.run('c5', 2 if rig else 5, 1 if rig else 4, events_after=True)[0])
                except Exception as e:      # noqa: BLE001
                    others['c5'] = {'error': f'{type(e).__name__}: {str(e).splitlines()[0][:200]}'}
    if r.rank == 0:
        out = {'metric': 'rollout-steps/sec (batch x horizon) on 256x256 terrain', 'value': res['value'], 'unit': 'rollout-steps/s',
               'n_gpus': r.world, 'world_size': r.dist_world, 'backend': ('rccl' if r.backend == 'nccl' else r.backend) if r.dist_on else None,
               'steps': res['steps'], 'warmup': res['warmup'], 'ms_per_step': res['ms_per_step'],
               'ms_per_step_ranks': res['ms_per_step_ranks'], 'comm_ms': res['comm_ms'],
               'higher_is_better': True, 'scaling': res['scaling'], 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
               'config': res['config'], **({'roofline': res['roofline']} if 'roofline' in res else {})}
        out.update(extras)
        if others:
            out['other_workloads'] = others
        if args.full and not args.no_cpu_baseline:
            out['cpu_baseline'] = cpu_baseline(N, args.integrator, T, headline=args.workload) if not r.dist_on else None      # timed at N=1 only
        detail_file = None
        if args.full:
            try:
                with open(args.detail, 'w') as f:
                    json.dump(out, f)
                detail_file = os.path.relpath(args.detail, REPO) if os.path.abspath(args.detail).startswith(REPO + os.sep) else args.detail
            except OSError as e:
                print(f'bench.py: could not write {args.detail}: {e}', file=sys.stderr)
        line = compact_line(out, detail_file)
    if r.dist_on:
        import torch.distributed as dist
        dist.destroy_process_group()      # (before the line: whatever the collective library says on its way out must not follow it)
    if r.rank == 0:
        # (RCCL announces itself with a C printf -- 'Librccl path : ...' -- that sits in the C library's buffer while stdout is a pipe and would
        #  come out at exit, BEHIND the line: flush every C stream first)
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        print(line, flush=True)      # the LAST stdout line, < 4 KB: what the driver parses


if __name__ == '__main__':
    main()
