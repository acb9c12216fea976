"""Cycle accounting of the streaming backward (A/B build with -DMF_STREAM_PROFILE: tools/build_variant.sh prof "-DMF_STREAM_PROFILE"
rollout_bwd_cp_stream_fast.hip; run with MONOFORCE_HIP_LIB=gpurun_in_ab/prof/libmonoforce_hip.so): per launch and workgroup, the
cycles the fetching waves spend waiting for room in the ring / for their turn to publish / in total, and the cycles the computing wave
waits for steps / runs in total; and where the computing wave's time outside its loop goes: kernel start -> first step in hand (fill),
after the last step the loss value's finish, the flush of its cell accumulators and the terrain snap.  AB_B=256,1024.
AB_WORKLOAD=c3 (default): the bench's fit step (TerrainFitProblem: forward, fused physics_loss with its value formed in the backward,
backward to the terrain), launched call by call; AB_WORKLOAD=plain: a positions-only loss outside the kernels."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from bench import build_problem
from monoforce_amd import _lib, _timing
L = _lib.lib()
NSLOT = 32
workload = os.environ.get('AB_WORKLOAD', 'c3')
for B in [int(x) for x in os.environ.get('AB_B', '256,1024,2048').split(',')]:
    cfg, dp, pts, masks, z, mu, ctrl = build_problem(B, 500, 4, 'cuda', 1)
    cd = ctrl.cuda()
    zl, ml = z.cuda().clone().requires_grad_(True), mu.cuda().clone().requires_grad_(True)
    if workload == 'c3':
        from monoforce_amd.train import TerrainFitProblem
        from monoforce_amd import synthetic as syn
        prob = TerrainFitProblem(dp, syn.bump_terrain(syn.bump_params(100), 6.4, 0.05).cuda(), mu.cuda(), cd, graph=False)

        def step():
            prob.step(zl, ml, eager=True)
    else:
        dp.return_forces = False

        def step():
            (Xs, _, _, _), _ = dp(zl.unsqueeze(0), cd, friction=ml.unsqueeze(0))
            (Xs[:, ::10] ** 2).mean().backward()
    step(); step(); torch.cuda.synchronize()
    L.mf_debug_stream_profile(None, 1)
    n = 4
    _timing.start()
    for _ in range(n): step()
    k = {nm: float(np.mean(v)) for nm, v in _timing.stop().items()}
    torch.cuda.synchronize()
    out = (C.c_ulonglong * NSLOT)()
    assert L.mf_debug_stream_profile(out, 0) == 0
    L.mf_debug_stream_profile(None, 1)      # one more launch alone: the extent of ONE launch from the 100 MHz clock
    step(); torch.cuda.synchronize()
    one = (C.c_ulonglong * NSLOT)()
    assert L.mf_debug_stream_profile(one, 0) == 0
    wg = (B + 3) // 4
    per = [v / (n * wg) for v in out]      # shader-clock ticks per launch and workgroup (sums); slots 13-15, 17: maxima
    mhz = 100.0 * out[12] / max(out[16], 1)       # the computing wave's cycles over its 100 MHz wall ticks: the shader clock
    span_us = (one[14] - (~one[15] & 0xFFFFFFFFFFFFFFFF)) / 100.0      # one launch: last wave's end - first wave's start
    print(f'{workload} B {B}: bwd {k.get("rollout_bwd_kernel", float("nan")):.4f} ms (HIP events) | shader clock {mhz:.0f} MHz | '
          f'one launch: first wave start -> last wave end {span_us:.1f} us', flush=True)
    print(f'  fetcher0 room {per[0]:.0f} publish {per[1]:.0f} total {per[2]:.0f} first step published at {per[18]:.0f} | '
          f'fetcher1 room {per[4]:.0f} publish {per[5]:.0f} total {per[6]:.0f}', flush=True)
    print(f'  compute: start -> first step in hand {per[3]:.0f} (of it waiting for the ring {per[19]:.0f}) | first step -> last step '
          f'{per[20] - per[3]:.0f}, of it waiting for the ring {per[8] - per[19]:.0f} (first 30 steps {per[22]:.0f}, last 30 {per[24]:.0f}; '
          f'{per[23]:.0f} waits of {max(496 // 2, 1)} pairs)', flush=True)
    print(f'  compute tail {per[12] - per[20]:.0f}: waiting for the snap cell {per[7]:.0f} | flush + emit '
          f'{per[10]:.0f} | snap {per[11]:.0f} | rest {per[12] - per[20] - per[7] - per[10] - per[11]:.0f}', flush=True)
    print(f'  loss value finish on fetcher0 {per[21]:.0f} (max over workgroups {out[17]:.0f})', flush=True)
    # (hand-off kernels: after its last step a fetching wave waits for the computing wave's last answer before it drains its slots)
    print(f'  fetchers waiting for the last answer: fetcher0 {per[25]:.0f} fetcher1 {per[26]:.0f}', flush=True)
    print(f'  compute wave start -> end {per[12]:.0f} (max over workgroups {out[13]:.0f})  (ticks per launch and workgroup)', flush=True)
