"""`hm_loss` (scripts/train.py:388-398, eval.py:146-147) and `total_variation` (scripts/fit_terrain.py:58): the HIP route (`mf_hm_loss_value_*` /
`mf_hm_loss_bwd_*`, `mf_total_variation_value_*` / `mf_total_variation_bwd_*`) against the ATen forms (`hm_loss_aten`, `total_variation_aten`:
the route of these calls before the kernels existed).

    python tools/bench_map_losses.py [--iters 60] [--warmup 10] [--out profiles/map_losses.txt]

Shapes: `hm_loss` on a [B,1,256,256] prediction with the labels as `[:, 0:1]` / `[:, 1:2]` channel views of a [B,2,256,256] tensor (a tenth of
the label cells NaN), B = 1 and 8, float32; total variation on a [256,256] map.
    value          the scalar, no autograd graph
    value_bwd      the scalar and its gradient with respect to the prediction / the map
    value_bwd_graph  the same captured once and replayed as a hipGraph: the kernels without the host's launch calls (what a captured
                   train or fit step pays)
Method: HIP events around every call, the forms alternating in one process after a warm-up of all of them; median, minimum and p90 over the calls.
Lines that other runs add to the output file (the headline bench.py and the encoder step before and after) are kept: only this tool's own block,
between its two marker lines, is replaced."""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from monoforce_amd import losses as L  # noqa: E402

DEV = 'cuda'
BEGIN, END = '# ---- tools/bench_map_losses.py: begin ----', '# ---- tools/bench_map_losses.py: end ----'


def alternate(forms, iters, warmup):
    """forms: dict name -> callable.  HIP events around every call, the forms alternating; returns dict name -> ms array."""
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for k in forms}
    for i in range(iters):
        for k, fn in forms.items():
            a, b = ev[k][i]
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    return {k: np.array([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}


def captured(fn):
    """`fn` captured into a hipGraph after two warm-up calls on the capture stream (its ticket and workspaces exist)."""
    from monoforce_amd.capture import capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with capture(g, stream=s, capture_error_mode='thread_local'):
        _KEEP.append(fn())       # (the replays write into these tensors)
    return g


_KEEP = []


def stats(ms):
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(ms.min()), 4), p90_ms=round(float(np.percentile(ms, 90)), 4))


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'map_losses.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_map_losses needs the MI355X'
    lines = [BEGIN,
             '# hm_loss on [B,1,256,256] float32 with channel-view labels ([:, 0:1] / [:, 1:2] of [B,2,256,256], a tenth of them NaN) and',
             '# total_variation on [256,256]: the HIP route (one launch forward, one backward) vs hm_loss_aten / total_variation_aten',
             f'# HIP events per call, forms alternating in one process, {args.warmup} warm-up + {args.iters} timed calls each; ms',
             f'# device: {torch.cuda.get_device_name(0)}']
    gen = torch.Generator().manual_seed(0)
    verdicts = []
    cases = []
    for B in (1, 8):
        pred = (0.5 * torch.randn(B, 1, 256, 256, generator=gen)).to(DEV).requires_grad_(True)
        labels = torch.stack([0.5 * torch.randn(B, 256, 256, generator=gen), 0.5 + torch.rand(B, 256, 256, generator=gen)], dim=1)
        labels[:, 0][torch.rand(B, 256, 256, generator=gen) < 0.1] = float('nan')
        labels = labels.to(DEV)
        cases.append((f'hm_loss {B}x256x256', dict(what='hm_loss', B=B, H=256, W=256), pred,
                      lambda fn, pred=pred, labels=labels: fn(pred, labels[:, 0:1], labels[:, 1:2]), (L.hm_loss, L.hm_loss_aten), '_FusedHmLoss'))
    z = (0.3 * torch.randn(256, 256, generator=gen)).to(DEV).requires_grad_(True)
    cases.append(('total_variation 256x256', dict(what='total_variation', H=256, W=256), z, lambda fn, z=z: fn(z),
                  (L.total_variation, L.total_variation_aten), '_FusedTotalVariation'))
    for title, row0, leaf, call, (hip, aten), node in cases:
        def value(fn):
            with torch.no_grad():
                return call(fn)

        def value_bwd(fn):
            loss = call(fn)
            return (loss,) + torch.autograd.grad(loss, (leaf,))
        forms = dict(hip_value=lambda: value(hip), aten_value=lambda: value(aten), hip_value_bwd=lambda: value_bwd(hip),
                     aten_value_bwd=lambda: value_bwd(aten))
        graphs = {k: captured(lambda fn=fn: value_bwd(fn)) for k, fn in (('hip', hip), ('aten', aten))}      # (kept alive: the forms replay them)
        forms.update(hip_value_bwd_graph=graphs['hip'].replay, aten_value_bwd_graph=graphs['aten'].replay)
        h, a = forms['hip_value_bwd'](), forms['aten_value_bwd']()
        assert type(h[0].grad_fn).__name__.startswith(node) and not type(a[0].grad_fn).__name__.startswith(node)
        dev = dict(loss=rel(h[0], a[0]), grad=float((h[1] - a[1]).abs().max() / a[1].abs().max()))
        assert all(math.isfinite(v) for v in dev.values()), dev
        ms = alternate(forms, args.iters, args.warmup)
        for k in forms:
            row = dict(row0, form=k, **stats(ms[k]))
            if k == 'hip_value_bwd':
                row.update(rel_dev_from_aten={n: float('%.3g' % v) for n, v in dev.items()})
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
        for k in ('value', 'value_bwd', 'value_bwd_graph'):
            ratio = float(np.median(ms['aten_' + k]) / np.median(ms['hip_' + k]))
            verdicts.append(ratio >= 1)
            lines.append(f'# {title}, {k}: aten / hip = {ratio:.2f} (median); the hip route is {"below" if ratio >= 1 else "NOT BELOW"} the ATen form')
            print(lines[-1], flush=True)
    lines.append('# the hip route is below the ATen form at every shape and form measured' if all(verdicts) else
                 '# the hip route is NOT below the ATen form everywhere: see the lines marked NOT BELOW')
    lines.append(END)
    kept = []
    if os.path.exists(args.out):      # what other runs recorded in the file stays
        old = open(args.out).read().split('\n')
        if BEGIN in old and END in old:
            old = old[:old.index(BEGIN)] + old[old.index(END) + 1:]
        kept = [ln for ln in old if ln.strip()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines + kept) + '\n')


if __name__ == '__main__':
    main()
