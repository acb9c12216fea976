"""`monoforce.transformations`: `position` and `transform_cloud`, the two functions of the reference's module that the label pipeline uses
(host code, numpy or torch).  Its Euler-angle and quaternion helpers need SciPy and are not provided."""
import numpy as np
import torch
from numpy.lib.recfunctions import structured_to_unstructured

__all__ = ['transform_cloud']


def position(cloud):
    """The xyz columns of a structured cloud as a plain array; a plain array is returned as it is."""
    return structured_to_unstructured(cloud[['x', 'y', 'z']]) if cloud.dtype.names else cloud


def transform_cloud(cloud, Tr):
    """The rigid transform `Tr` ([4,4], or [3,4]) applied to a cloud [N,3], numpy or torch: `R p + t` per point, in the promoted type of the
    two.  A structured numpy cloud comes back as a copy with its x, y, z fields replaced."""
    assert isinstance(cloud, (np.ndarray, torch.Tensor)), type(cloud)
    assert isinstance(Tr, (np.ndarray, torch.Tensor)), type(Tr)
    if isinstance(cloud, np.ndarray) and cloud.dtype.names is not None:
        moved = transform_cloud(position(cloud), Tr)
        out = cloud.copy()
        for k, name in enumerate('xyz'):
            out[name] = moved[:, k]
        return out
    assert cloud.ndim == 2 and cloud.shape[1] == 3, cloud.shape
    return (Tr[:3, :3] @ cloud.T + Tr[:3, 3:]).T
