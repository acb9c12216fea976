"""`monoforce.cloudproc` -> monoforce_amd.cloudproc (estimate_heightmap on the HIP kernel; filter_grid, hm_to_cloud, within_bounds on the host)."""
from monoforce_amd.cloudproc import *  # noqa: F401,F403
