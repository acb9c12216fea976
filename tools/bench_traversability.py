"""`traversability_map` on the MI355X: the HIP kernel (`mf_traversability_*`, one launch) against the ATen form (`traversability_map_aten`: pad,
unfold, gather, masked sums -- what a user would write without the kernel).

    python tools/bench_traversability.py [--iters 40] [--warmup 5] [--out profiles/traversability.txt]
    python tools/bench_traversability.py --metadata-only      (no GPU: refresh the kernel's metadata lines of an existing output file)

Shapes: 1 x 256 x 256 and 8 x 256 x 256 float32 maps (a tenth of the cells NaN), window radius r = 3, 7, 16 cells, with and without the term
layers.  Modes:
    launch   launch by launch, into static buffers (the kernel) / as the composition allocates (ATen)
    graph    the same call captured once and replayed as a hipGraph: the kernels without the host's launch calls
Method: HIP events around every call, the two forms alternating in one process after a warm-up of both; median, minimum and p90 over the
calls.  The kernel's register, LDS and scratch figures (tools/kernel_metadata.py) are recorded next to the times when the objects are there."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_map_losses import alternate, captured, stats  # noqa: E402
from monoforce_amd import costmap as cm  # noqa: E402

DEV = 'cuda'
RAMPS = dict(slope=cm.DEFAULT_SLOPE, roughness=cm.DEFAULT_ROUGHNESS, step=cm.DEFAULT_STEP)


def terrain(S, gen):
    i = torch.arange(256.0).view(1, 256, 1) * 0.1
    j = torch.arange(256.0).view(1, 1, 256) * 0.1
    z = 0.4 * torch.sin(0.7 * i) * torch.cos(0.5 * j) + 0.03 * torch.randn(S, 256, 256, generator=gen)
    z[torch.rand(S, 256, 256, generator=gen) < 0.1] = float('nan')
    return z.to(DEV)


def metadata_lines():
    try:
        import kernel_metadata
        return ['# ' + json.dumps(dict(kernel=name, **m)) for o, name, m in kernel_metadata.kernels() if o == 'traversability.o']
    except Exception as e:      # (no LLVM tools)
        return [f'# kernel metadata not available here: {type(e).__name__}']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--metadata-only', action='store_true')
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'traversability.txt'))
    args = ap.parse_args()
    if args.metadata_only:
        old = [ln for ln in open(args.out).read().split('\n') if ln.strip() and not ln.startswith('# {"kernel"') and 'kernel metadata' not in ln]
        at = next(i for i, ln in enumerate(old) if ln.startswith('# device:')) + 1
        with open(args.out, 'w') as f:
            f.write('\n'.join(old[:at] + (metadata_lines() or ['# kernel metadata not available here: the objects are not built']) + old[at:]) + '\n')
        return
    assert torch.cuda.is_available(), 'bench_traversability needs the MI355X'
    lines = ['# traversability_map on [S,256,256] float32 (a tenth of the cells NaN), grid_res 0.1, default ramps: the HIP kernel (one launch,',
             '# static buffers) vs traversability_map_aten (pad + unfold + gather + masked sums)',
             f'# HIP events per call, forms alternating in one process, {args.warmup} warm-up + {args.iters} timed calls each; ms',
             f'# device: {torch.cuda.get_device_name(0)}']
    lines += metadata_lines() or ['# kernel metadata not available here: the objects are not next to the library (--metadata-only adds it)']
    gen = torch.Generator().manual_seed(0)
    verdicts = []
    for S in (1, 8):
        z = terrain(S, gen)
        for r in (3, 7, 16):
            for want_terms in (False, True):
                cost = torch.empty_like(z)
                terms = torch.empty(S, 3, 256, 256, device=DEV) if want_terms else None
                lo, hi = [v[0] for v in RAMPS.values()], [v[1] for v in RAMPS.values()]

                def hip():
                    return cm.traversability_into(z, None, None, 0.1, r, lo, hi, 0.5, 3, cost, terms)

                def aten():
                    return cm.traversability_map_aten(z, 0.1, radius_cells=r, return_terms=want_terms, **RAMPS)
                a = aten()
                a_cost = a[0] if want_terms else a
                hip()
                dev = float((cost - a_cost).abs().max())
                assert dev < 1e-4, dev
                forms = dict(hip_launch=hip, aten_launch=aten)
                graphs = {k: captured(fn) for k, fn in (('hip', hip), ('aten', aten))}
                forms.update(hip_graph=graphs['hip'].replay, aten_graph=graphs['aten'].replay)
                ms = alternate(forms, args.iters, args.warmup)
                for k in forms:
                    row = dict(S=S, H=256, W=256, r=r, terms=want_terms, form=k, **stats(ms[k]))
                    if k == 'hip_launch':
                        row['max_abs_dev_from_aten'] = float('%.3g' % dev)
                    lines.append(json.dumps(row))
                    print(lines[-1], flush=True)
                for k in ('launch', 'graph'):
                    ratio = float(np.median(ms['aten_' + k]) / np.median(ms['hip_' + k]))
                    verdicts.append(ratio >= 1)
                    lines.append(f'# {S}x256x256 r={r} terms={int(want_terms)}, {k}: aten / hip = {ratio:.1f} (median); the kernel is '
                                 f'{"below" if ratio >= 1 else "NOT BELOW"} the ATen form')
                    print(lines[-1], flush=True)
                del graphs, forms
                torch.cuda.empty_cache()
    lines.append('# the kernel is below the ATen form at every shape, radius and mode measured' if all(verdicts) else
                 '# the kernel is NOT below the ATen form everywhere: see the lines marked NOT BELOW')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
