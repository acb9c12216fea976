"""monoforce_amd: MI355X-native (gfx950) hot path of MonoForce -- DPhysics rollout + LSS BEV splat.

Importing the package is cheap and GPU-free; the HIP library (`monoforce_amd/csrc/libmonoforce_hip.so`)
is loaded on first use by `monoforce_amd._lib.lib()` and its absence is a hard error (no CPU fallback).
"""
__version__ = '0.1.0'


def __getattr__(name):
    """Lazy top-level names (keeps `import monoforce_amd` free of torch and of the HIP library)."""
    if name in ('DPhysics', 'generate_controls'):
        from . import dphysics
        return getattr(dphysics, name)
    if name == 'DPhysConfig':
        from .dphys_config import DPhysConfig
        return DPhysConfig
    if name == 'LiftSplatShoot':
        from .terrain_encoder import LiftSplatShoot
        return LiftSplatShoot
    if name == 'TrajectoryShooter':
        from .planner import TrajectoryShooter
        return TrajectoryShooter
    if name == 'MPPIPlanner':
        from .mppi import MPPIPlanner
        return MPPIPlanner
    if name == 'TerrainFitter':
        from .fit import TerrainFitter
        return TerrainFitter
    if name in ('ControlRefiner', 'trajectory_objective', 'trajectory_objective_aten'):
        from . import refine
        return getattr(refine, name)
    if name in ('TraversabilityMap', 'traversability_map', 'traversability_map_aten'):
        from . import costmap
        return getattr(costmap, name)
    if name in ('RoutePlanner', 'cost_to_go', 'extract_route', 'cost_to_go_aten', 'extract_route_host'):
        from . import route
        return getattr(route, name)
    if name in ('rigid_terrain_heightmap', 'rigid_terrain_heightmap_aten', 'semantic_cloud', 'footprint_traj_points'):
        from . import labels
        return getattr(labels, name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
