"""Referee of the rigid-terrain label maps: the definition in the comment of `MfTerrainLabelsDesc` (include/monoforce_hip.h) in numpy.  Never
imported by the product.  Float32 arithmetic is evaluated elementwise in the stated order (numpy rounds every array operation on its own); the
two rigid transforms are evaluated in float64 and rounded to float32 once."""
import numpy as np

f32, f64 = np.float32, np.float64


def class_mask(labels):
    """256 booleans from an iterable of labels 0..255."""
    m = np.zeros(256, dtype=bool)
    for v in labels:
        m[int(v)] = True
    return m


def project(p, R, t, K):
    """p [N,3], R [3,3], t [3], K [3,3], all float32 -> (u, v, w2), float32, in the definition's operation order."""
    p, R, t, K = (np.asarray(a, dtype=f32) for a in (p, R, t, K))
    with np.errstate(all='ignore'):
        a = [p[:, k] - t[k] for k in range(3)]
        q = [(R[0, i] * a[0] + R[1, i] * a[1]) + R[2, i] * a[2] for i in range(3)]
        w = [(K[i, 0] * q[0] + K[i, 1] * q[1]) + K[i, 2] * q[2] for i in range(3)]
        u, v = w[0] / w[2], w[1] / w[2]
    assert u.dtype == f32 and v.dtype == f32 and w[2].dtype == f32
    return u, v, w[2]


def seen_mask(u, v, w2, Hi, Wi):
    with np.errstate(invalid='ignore'):
        return (w2 > f32(0)) & (u > f32(1)) & (u < f32(Wi - 1)) & (v > f32(1)) & (v < f32(Hi - 1))


def point_labels(p, seg, rots, trans, intrins):
    """p [N,3]; seg [C,Hi,Wi] uint8; cameras [C,...] -> int16 [N,C], -1 where the camera does not see the point."""
    C, Hi, Wi = seg.shape
    out = np.full((p.shape[0], C), -1, dtype=np.int16)
    for c in range(C):
        u, v, w2 = project(p, rots[c], trans[c], intrins[c])
        m = seen_mask(u, v, w2, Hi, Wi)
        out[m, c] = seg[c][v[m].astype(np.int64), u[m].astype(np.int64)]       # astype of a positive float truncates
    return out


def rigid_transform(P, x, y, z, tz_off=0.0):
    """[3,4] float64 pose applied to float coordinates in float64, ((r0 x + r1 y) + r2 z) + t per row, rounded to float32 -> [N,3]."""
    P = np.asarray(P, dtype=f64)
    x, y, z = (np.asarray(a).astype(f64) for a in (x, y, z))
    t = [P[0, 3], P[1, 3], P[2, 3] - abs(f64(tz_off))]
    with np.errstate(all='ignore'):
        return np.stack([(((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + t[r]).astype(f32) for r in range(3)], axis=1)


def footprint_points(poses, fx, fy, clearance):
    """poses [T,3,4] float64; -> [T*Fy*Fx, 3] float32 in the order (t, j, i) of the definition."""
    fx, fy = np.asarray(fx, dtype=f32), np.asarray(fy, dtype=f32)
    X, Y = np.meshgrid(fx, fy)                  # rows are y
    X, Y = X.reshape(-1), Y.reshape(-1)
    out = [rigid_transform(P, X, Y, np.zeros_like(X), clearance) for P in np.asarray(poses, dtype=f64).reshape(-1, 3, 4)]
    return np.concatenate(out, axis=0) if out else np.zeros((0, 3), dtype=f32)


def heightmap(g, bins, d_max, h_min, h_max, r_min=None):
    """estimate_heightmap's definition on float32 points g [M,3] -> [2,n,n] float32."""
    g = np.asarray(g, dtype=f32)
    bins = np.asarray(bins, dtype=f32)
    n = bins.size
    with np.errstate(invalid='ignore'):
        g = g[~np.isnan(g).any(axis=1)]
        if r_min is not None and r_min >= 0:
            dist = np.sqrt(g[:, 0].astype(f64) * g[:, 0].astype(f64) + g[:, 1].astype(f64) * g[:, 1].astype(f64)).astype(f32)
            g = g[dist > f32(r_min)]
        d, lo, hi = f32(d_max), f32(h_min), f32(h_max)
        g = g[(g[:, 0] > -d) & (g[:, 0] < d) & (g[:, 1] > -d) & (g[:, 1] < d) & (g[:, 2] > lo) & (g[:, 2] < hi)]
    ix = np.searchsorted(bins, g[:, 0], side='left') - 1       # edges strictly below x, minus one
    iy = np.searchsorted(bins, g[:, 1], side='left') - 1
    ok = (ix >= 0) & (iy >= 0)
    ix, iy, z = ix[ok], iy[ok], g[ok, 2]
    # the maximum in the total order of the bit patterns (-0.0 below +0.0), which is what an integer maximum on the ordered key gives
    b = np.ascontiguousarray(z).view(np.int32)
    key = np.where(b >= 0, b, b ^ np.int32(0x7FFFFFFF))
    top = np.full((n, n), np.iinfo(np.int32).min, dtype=np.int32)
    np.maximum.at(top, (ix, iy), key)
    got = top != np.iinfo(np.int32).min
    val = np.where(top >= 0, top, top ^ np.int32(0x7FFFFFFF)).astype(np.int32).view(f32)
    return np.stack([np.where(got, val, f32(0)), got.astype(f32)]).astype(f32)


def terrain_labels(points, offsets, seg, rots, trans, intrins, rigid_labels, pose_align, poses, fx, fy, clearance, bins, d_max, h_max,
                   h_min=None, r_min=None):
    """points [sumN,3] f32; offsets [S+1]; seg [S,C,Hi,Wi] u8; rots/trans/intrins [S,C,..] or [C,..] (shared); pose_align [S,3,4] f64;
    poses [S,T,3,4] f64 -> (hm [S,2,n,n] f32, point_labels [sumN,C] i16)."""
    points = np.asarray(points, dtype=f32).reshape(-1, 3)
    S, C = seg.shape[0], seg.shape[1]
    member = class_mask(rigid_labels)
    labels = np.full((points.shape[0], C), -1, dtype=np.int16)
    hms = []
    for s in range(S):
        p = points[offsets[s]:offsets[s + 1]]
        cam = [a if a.ndim == b else a[s] for a, b in ((np.asarray(rots), 3), (np.asarray(trans), 2), (np.asarray(intrins), 3))]
        lab = point_labels(p, seg[s], *cam)
        lab[np.isnan(p).any(axis=1)] = -1                      # the NaN rule comes before the projection
        labels[offsets[s]:offsets[s + 1]] = lab
        kept = (member[np.maximum(lab, 0)] & (lab >= 0)).any(axis=1) if C else np.zeros(p.shape[0], dtype=bool)
        pk = p[kept]
        g = rigid_transform(pose_align[s], pk[:, 0], pk[:, 1], pk[:, 2])
        g = np.concatenate([g, footprint_points(poses[s], fx, fy, clearance)], axis=0)
        hms.append(heightmap(g, bins, d_max, -h_max if h_min is None else h_min, h_max, r_min))
    return np.stack(hms), labels
