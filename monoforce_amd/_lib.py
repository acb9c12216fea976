"""ctypes binding of libmonoforce_hip.so (the C ABI declared in include/monoforce_hip.h).

There is no CPU fallback: if the library has not been built (`python -c "import __graft_entry__ as g; g.build()"`
or `make -C monoforce_amd/csrc`) every entry point raises.

`launch` is the ONE way a kernel entry point is called: the tensors' device current, the optional `_timing` bracket, the dtype suffix,
tensors -> pointers (`c_args`), the current stream last, `check` (one exception, `rollout_launch.GradPool.reduce`: the stream it was
acquired on, not the current one).  `size_query` is the same for the two byte-count queries.  WHICH
arguments an entry point takes is written down once, in the module that owns it: rollout_launch.py (`mf_rollout_*`,
`mf_reduce_grad_copies_*`), splat.py (`mf_bev_*`), losses.py (`mf_physics_loss_*`, `mf_pose_loss_*`, `mf_nearest_steps_*`, `mf_hm_loss_*`, `mf_total_variation_*`),
terrain_stage.py, cloudproc.py, fit.py (`mf_terrain_fit_*`), refine.py (`mf_traj_objective_*`, `mf_control_refine_update_*`), dphysics.py (`mf_interpolate_grid_*`), costmap.py (`mf_traversability_*`), route.py (`mf_cost_to_go_*`, `mf_extract_route_*`), labels.py (`mf_terrain_labels_*`), ops.py (MPPI and pose costs); tests/test_capi_cpu.py holds
the tree to that.  Importing this module loads nothing: the library comes in at the first `lib()`.
"""
import contextlib
import ctypes as C
import os
import threading

import torch

from . import _timing

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libmonoforce_hip.so')

MF_INTEG_DYNAMICS, MF_INTEG_ODEINT_EULER = 0, 1
MF_LAYOUT_BATCH_MAJOR, MF_LAYOUT_TIME_MAJOR = 0, 1
MF_LOSS_VALUE_IN_BACKWARD = 1
# the answers of mf_rollout_loss_fusable: neither launch carries the loss / both do / the backward alone, of a saturated
# positions-only launch / the backward alone, of a component-parallel launch in its early-recompute form
MF_LOSS_FUSE_NONE, MF_LOSS_FUSE_BOTH, MF_LOSS_FUSE_BACKWARD_SATURATED, MF_LOSS_FUSE_BACKWARD_EARLY = 0, 1, 2, 3
MF_MATH_EXACT, MF_MATH_FAST = 0, 1
MF_LANES_COMPONENT = 16


class MfRolloutDesc(C.Structure):
    _fields_ = [('B', C.c_int32), ('T', C.c_int32), ('N', C.c_int32), ('H', C.c_int32), ('W', C.c_int32),
                ('n_tracks', C.c_int32), ('integrator', C.c_int32), ('layout', C.c_int32), ('map_shared', C.c_int32),
                ('block', C.c_int32), ('skip_snap', C.c_int32), ('points_per_lane', C.c_int32), ('math_mode', C.c_int32), ('force_stride', C.c_int32), ('grad_copies', C.c_int32), ('has_joints', C.c_int32), ('pose_stride', C.c_int32), ('cost_project', C.c_int32), ('default_state', C.c_int32), ('controls_stride_b', C.c_int32), ('controls_stride_t', C.c_int32),
                ('mass', C.c_double), ('gravity', C.c_double), ('stiffness', C.c_double), ('damping', C.c_double),
                ('omega_max', C.c_double), ('grid_res', C.c_double), ('d_max', C.c_double), ('dt', C.c_double),
                ('robot_size_y', C.c_double), ('Iinv', C.c_double * 9), ('joint_xyz', C.c_double * 12)]


class MfRolloutLoss(C.Structure):
    _fields_ = [('T2', C.c_int32), ('flags', C.c_int32)] + [(n, C.c_void_p) for n in ('gt', 'near', 'w', 'row_stamp', 'row_w', 'partial', 'ticket', 'loss', 'gloss', 'Xs')]


class MfRolloutFwdBufs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('z', 'mu', 'controls', 'ts', 'points', 'part', 'x0', 'xd0', 'R0', 'w0',
                                          'Xs', 'Xds', 'Rs', 'Omegas', 'Fs', 'Ff', 'Xraw', 'joint_angles', 'cost_rows', 'path_cost',
                                          'zmu_scratch', 'zmu', 'rec', 'loss')]


class MfRolloutBwdBufs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('z', 'mu', 'controls', 'ts', 'points', 'part', 'x_init', 'xd0', 'R0', 'w0',
                                          'Xraw', 'Xds', 'Rs', 'Omegas',
                                          'gXs', 'gXds', 'gRs', 'gOmegas', 'gFs', 'gFf', 'zeros',
                                          'gz', 'gmu', 'gcontrols', 'gx0', 'gxd0', 'gR0', 'gw0', 'joint_angles', 'gjoint_angles', 'rec', 'loss',
                                          'zmu_scratch', 'zmu')]


class MfLossDesc(C.Structure):
    _fields_ = [('B', C.c_int32), ('T1', C.c_int32), ('T2', C.c_int32), ('reserved', C.c_int32),
                ('x_stride_b', C.c_int64), ('x_stride_t', C.c_int64), ('gamma', C.c_double)]


class MfSplatDesc(C.Structure):
    _fields_ = [('B', C.c_int32), ('n_per_sample', C.c_int32), ('C', C.c_int32),
                ('nx', C.c_int32), ('ny', C.c_int32), ('nz', C.c_int32),
                ('off', C.c_float * 3), ('dx', C.c_float * 3), ('lift_D', C.c_int32), ('lift_hw', C.c_int32)]


class MfStageDesc(C.Structure):
    _fields_ = [('B', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('k', C.c_int32)]


class MfInterpDesc(C.Structure):
    _fields_ = [('B', C.c_int32), ('N', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('map_shared', C.c_int32), ('math_mode', C.c_int32),
                ('grid_res', C.c_double), ('d_max', C.c_double)]


class MfHeightmapDesc(C.Structure):
    _fields_ = [('n_points', C.c_int32), ('nx', C.c_int32), ('ny', C.c_int32), ('d_max', C.c_float), ('h_min', C.c_float),
                ('h_max', C.c_float), ('r_min', C.c_float), ('inv_res', C.c_float)]


class MfMppiDesc(C.Structure):
    # (`lam` is the header's `lambda`)
    _fields_ = [('B', C.c_int32), ('T', C.c_int32), ('keep_nominal', C.c_int32), ('reserved', C.c_int32),
                ('row_stride_b', C.c_int64), ('row_stride_t', C.c_int64), ('x_stride_b', C.c_int64),
                ('sigma', C.c_float * 2), ('lo', C.c_float * 2), ('hi', C.c_float * 2),
                ('w_incl', C.c_float), ('w_force', C.c_float), ('w_goal', C.c_float), ('lam', C.c_float)]


class MfPoseCostDesc(C.Structure):
    _fields_ = [('B', C.c_int32), ('Tp', C.c_int32), ('N', C.c_int32), ('P', C.c_int32), ('H', C.c_int32), ('W', C.c_int32),
                ('x_stride_b', C.c_int64), ('x_stride_t', C.c_int64), ('r_stride_b', C.c_int64), ('r_stride_t', C.c_int64),
                ('grid_res', C.c_float), ('d_max', C.c_float), ('lethal', C.c_float), ('off_map', C.c_float), ('w_map', C.c_float), ('w_path', C.c_float)]


class MfPoseLossDesc(C.Structure):
    _fields_ = [('B', C.c_int32), ('T1', C.c_int32), ('T2', C.c_int32), ('reserved', C.c_int32),
                ('x_stride_b', C.c_int64), ('x_stride_t', C.c_int64), ('r_stride_b', C.c_int64), ('r_stride_t', C.c_int64), ('gamma', C.c_double)]


class MfMapLossDesc(C.Structure):
    _fields_ = [('M', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('use_h_max', C.c_int32),
                ('p_stride_m', C.c_int64), ('p_stride_h', C.c_int64), ('g_stride_m', C.c_int64), ('g_stride_h', C.c_int64),
                ('w_stride_m', C.c_int64), ('w_stride_h', C.c_int64), ('o_stride_m', C.c_int64), ('o_stride_h', C.c_int64), ('h_max', C.c_double)]


MF_FIT_CLAMP_Z, MF_FIT_CLAMP_MU = 1, 2


class MfFitDesc(C.Structure):
    _fields_ = [('n_z', C.c_int64), ('n_mu', C.c_int64), ('max_iters', C.c_int32), ('flags', C.c_int32),
                ('lr_z', C.c_double), ('lr_mu', C.c_double), ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double),
                ('z_lo', C.c_double), ('z_hi', C.c_double), ('mu_lo', C.c_double), ('mu_hi', C.c_double)]


class MfTrajObjDesc(C.Structure):
    _fields_ = [('B', C.c_int32), ('T', C.c_int32), ('N', C.c_int32), ('P', C.c_int32), ('H', C.c_int32), ('W', C.c_int32),
                ('pose_stride', C.c_int32), ('reserved', C.c_int32),
                ('x_stride_b', C.c_int64), ('x_stride_t', C.c_int64), ('r_stride_b', C.c_int64), ('r_stride_t', C.c_int64),
                ('grid_res', C.c_float), ('d_max', C.c_float), ('lethal', C.c_float), ('off_map', C.c_float),
                ('w_map', C.c_float), ('w_path', C.c_float), ('w_goal', C.c_float), ('w_incl', C.c_float)]


class MfRefineDesc(C.Structure):
    _fields_ = [('K', C.c_int32), ('T', C.c_int32), ('max_iters', C.c_int32), ('reserved', C.c_int32),
                ('lr', C.c_double * 2), ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double),
                ('lo', C.c_float * 2), ('hi', C.c_float * 2)]


MF_TRAVERSABILITY_TILE, MF_TRAVERSABILITY_MAX_RADIUS = 16, 16


class MfTraversabilityDesc(C.Structure):
    _fields_ = [('S', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('r', C.c_int32), ('min_valid', C.c_int32), ('reserved', C.c_int32),
                ('z_stride_s', C.c_int64), ('z_stride_h', C.c_int64), ('v_stride_s', C.c_int64), ('v_stride_h', C.c_int64),
                ('b_stride_s', C.c_int64), ('b_stride_h', C.c_int64), ('grid_res', C.c_float), ('unknown', C.c_float),
                ('lo', C.c_float * 3), ('hi', C.c_float * 3)]


class MfTerrainLabelsDesc(C.Structure):
    _fields_ = [('S', C.c_int32), ('C', C.c_int32), ('Hi', C.c_int32), ('Wi', C.c_int32), ('T', C.c_int32), ('Fx', C.c_int32), ('Fy', C.c_int32),
                ('n', C.c_int32), ('n_points', C.c_int32), ('max_points', C.c_int32),
                ('rots_stride_s', C.c_int64), ('trans_stride_s', C.c_int64), ('intrins_stride_s', C.c_int64),
                ('class_set', C.c_uint32 * 8), ('clearance', C.c_double),
                ('d_max', C.c_float), ('h_min', C.c_float), ('h_max', C.c_float), ('r_min', C.c_float), ('inv_res', C.c_float), ('reserved', C.c_int32)]


MF_ROUTE_TILE, MF_ROUTE_MAX_VERTICES = 32, 256
MF_ROUTE_GOAL_BLOCKED, MF_ROUTE_NOT_CONVERGED, MF_ROUTE_START_UNREACHABLE, MF_ROUTE_TRUNCATED = 1, 2, 4, 8


class MfCostToGoDesc(C.Structure):
    _fields_ = [('S', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('n_rounds', C.c_int32), ('c_stride_s', C.c_int64), ('c_stride_h', C.c_int64),
                ('grid_res', C.c_float), ('d_max', C.c_float), ('lethal', C.c_float), ('alpha', C.c_float)]


class MfRouteDesc(C.Structure):
    _fields_ = [('S', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('P', C.c_int32), ('max_nodes', C.c_int32), ('reserved', C.c_int32),
                ('c_stride_s', C.c_int64), ('c_stride_h', C.c_int64),
                ('grid_res', C.c_float), ('d_max', C.c_float), ('lethal', C.c_float), ('alpha', C.c_float)]


# every symbol include/monoforce_hip.h declares; tests check the library exports all of them
SYMBOLS = ['mf_rollout_force_stride', 'mf_rollout_fwd_f32', 'mf_rollout_fwd_f64', 'mf_rollout_default_state_f32', 'mf_rollout_default_state_f64', 'mf_rollout_bwd_f32', 'mf_rollout_bwd_f64', 'mf_rollout_bwd_wants_gcontrols', 'mf_rollout_record_bytes', 'mf_rollout_record_bytes_f64', 'mf_rollout_fwd_stages_zmu', 'mf_rollout_loss_fusable', 'mf_rollout_bwd_window', 'mf_bev_splat_workspace_bytes', 'mf_bev_splat_prepare', 'mf_bev_splat_prepare_cameras', 'mf_bev_splat_prepare_rig',
           'mf_bev_splat_fwd_f32', 'mf_bev_splat_fwd_f64', 'mf_bev_splat_bwd_f32', 'mf_bev_splat_bwd_f64',
           'mf_bev_lift_splat_fwd_f32', 'mf_bev_lift_splat_fwd_f64', 'mf_bev_lift_splat_bwd_f32', 'mf_bev_lift_splat_bwd_f64',
           'mf_physics_loss_fwd_f32', 'mf_physics_loss_fwd_f64', 'mf_physics_loss_bwd_f32', 'mf_physics_loss_bwd_f64', 'mf_physics_loss_value_f32', 'mf_physics_loss_value_f64', 'mf_nearest_steps_f32', 'mf_nearest_steps_f64', 'mf_reduce_grad_copies_f32', 'mf_reduce_grad_copies_f64', 'mf_estimate_heightmap_f32', 'mf_interpolate_grid_f32', 'mf_interpolate_grid_f64', 'mf_terrain_stage_fwd_f32', 'mf_terrain_stage_bwd_f32', 'mf_mppi_perturb_f32', 'mf_path_costs_f32', 'mf_mppi_scratch_bytes', 'mf_mppi_update_f32', 'mf_pose_costs_f32', 'mf_pose_loss_value_f32', 'mf_pose_loss_value_f64', 'mf_pose_loss_bwd_f32', 'mf_pose_loss_bwd_f64', 'mf_hm_loss_value_f32', 'mf_hm_loss_value_f64', 'mf_hm_loss_bwd_f32', 'mf_hm_loss_bwd_f64', 'mf_total_variation_value_f32', 'mf_total_variation_value_f64', 'mf_total_variation_bwd_f32', 'mf_total_variation_bwd_f64', 'mf_terrain_fit_update_f32', 'mf_terrain_fit_update_f64', 'mf_terrain_fit_grid_cap', 'mf_traj_objective_f32', 'mf_control_refine_update_f32', 'mf_traversability_f32', 'mf_traversability_f64', 'mf_cost_to_go_work_ints', 'mf_cost_to_go_f32', 'mf_cost_to_go_f64', 'mf_extract_route_f32', 'mf_extract_route_f64', 'mf_terrain_labels_f32', 'mf_last_error', 'mf_last_launch', 'mf_version', 'mf_sizeof']

_lib = None
_lock = threading.Lock()


def lib():
    """Load (once) and return the HIP library; raise loudly if it is not there."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f'{LIB_PATH} is missing: build the HIP extension first (make -C monoforce_amd/csrc). '
                        'monoforce_amd has no CPU fallback.')
                # torch bundles its own libamdhip64.so.7; it is imported FIRST (above) so this library binds to the same HIP runtime
                # instance (loading /opt/rocm's copy first leaves the process with two runtimes and no device).
                L = C.CDLL(os.environ.get('MONOFORCE_HIP_LIB', LIB_PATH))   # override: A/B builds of the kernels (tools/)
                L.mf_last_error.restype = C.c_char_p
                L.mf_version.restype = C.c_char_p
                L.mf_last_launch.restype = C.c_char_p
                for name in SYMBOLS:
                    fn = getattr(L, name)   # AttributeError if the build is stale
                    if name.startswith(('mf_rollout', 'mf_bev', 'mf_physics', 'mf_estimate', 'mf_terrain_stage', 'mf_terrain_fit', 'mf_terrain_labels', 'mf_reduce', 'mf_interpolate', 'mf_nearest', 'mf_mppi', 'mf_path', 'mf_pose', 'mf_hm_loss', 'mf_total_variation', 'mf_traj', 'mf_control', 'mf_traversability', 'mf_cost_to_go', 'mf_extract_route')):
                        fn.restype = C.c_int
                L.mf_bev_splat_workspace_bytes.restype = C.c_size_t
                L.mf_rollout_record_bytes.restype = C.c_longlong
                L.mf_rollout_record_bytes_f64.restype = C.c_longlong
                L.mf_mppi_scratch_bytes.restype = C.c_longlong
                L.mf_cost_to_go_work_ints.restype = C.c_longlong
                _lib = L
    return _lib


ON_ERROR = []      # callables run when an entry point reports an error (state that assumed the launch completed is dropped)


def check(rc, what):
    if rc != 0:
        for fn in list(ON_ERROR):
            fn()
        raise RuntimeError(f'{what} failed (code {rc}): {lib().mf_last_error().decode()}')


def size_query(entry, desc):
    """A byte-count query `entry(desc)` (not a launch: no device, no stream); the library answers a bad descriptor with 0 or -1 and
    leaves the reason in mf_last_error."""
    nbytes = int(getattr(lib(), entry)(C.byref(desc)))
    if nbytes <= 0:
        raise RuntimeError(f'{entry}: {lib().mf_last_error().decode()}')
    return nbytes


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def scalar_suffix(dtype):
    if dtype == torch.float32:
        return 'f32'
    if dtype == torch.float64:
        return 'f64'
    raise TypeError(f'the HIP kernels compute in float32 or float64, got {dtype}')


def stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def c_args(*args):
    """Arguments as the C ABI takes them: a tensor -> its device pointer, a descriptor (`ctypes.Structure`) -> by reference; None (NULL),
    ctypes scalars and arrays pass as they are."""
    return [C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else C.byref(a) if isinstance(a, C.Structure) else a for a in args]


def launch(entry, device, *args, dtype=None, timer=None):
    """Call the kernel entry point `entry` (`dtype`: its `_f32` / `_f64` variant) on `device`'s current stream, with that device
    CURRENT -- the library's policy reads the current device's CU count -- and, with `timer`, inside that `_timing`
    bracket.  `args` go through `c_args`; the stream is appended.  A failure raises with the un-suffixed name."""
    fn = getattr(lib(), entry if dtype is None else f'{entry}_{scalar_suffix(dtype)}')
    with torch.cuda.device(device), (_timing.timed(timer, device) if timer else contextlib.nullcontext()):
        check(fn(*c_args(*args), stream_ptr(device)), entry)


def require_hip_tensor(t, name):
    if not t.is_cuda:
        raise RuntimeError(f'{name} is on {t.device}: monoforce_amd computes on the MI355X HIP path only '
                           '(no CPU fallback); move inputs to "cuda".')
