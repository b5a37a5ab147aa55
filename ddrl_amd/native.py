"""ctypes binding of libddrl_hip.so (include/ddrl_hip.h).

The HIP library is the only compute path: if it is missing or fails to load, every entry
point raises.  There is no CPU fallback.  Device buffers are passed as raw pointers (for
example torch tensors' data_ptr()); torch is plumbing for memory and streams only.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libddrl_hip.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "ddrl_hip.h")

MAX_P, MAX_AG, MAX_OBS = 4, 4, 48
MODEL_FFN, MODEL_GNN = 0, 1
REWARD_PER_LEG, REWARD_GLOBAL, REWARD_NORM = 0, 1, 2
VF_CLIP_RAY10, VF_CLIP_SQUARED = 0, 1
# message-passing layer of the "gnn" model (models/graph_net.py:20 selects one of models/gcn.py's)
GNN_LAYERS = {"mpnn": 0, "gcn": 1, "mpnn2": 2, "gat1": 3}
RNG_NOISE, RNG_SCHEDULE = 0, 1   # DDRL_RNG_*: the two streams of a context's device generator
_U64 = (1 << 64) - 1

i32, f32 = C.c_int32, C.c_float


class DdrlCfg(C.Structure):
    _fields_ = [
        ("n_envs", i32), ("frag_len", i32), ("obs_full_dim", i32), ("n_agents", i32),
        ("n_policies", i32), ("model_kind", i32), ("act_dim", i32),
        ("agent_policy", i32 * MAX_AG), ("obs_dim", i32 * MAX_P),
        ("obs_index", (i32 * MAX_OBS) * MAX_AG), ("act_index", (i32 * 8) * MAX_AG),
        ("n_contact", i32 * MAX_AG), ("contact_index", (i32 * 14) * MAX_AG),
        ("contact_weight", (f32 * 14) * MAX_AG), ("leg_angle_deg", f32 * MAX_AG),
        ("filter_enabled", i32), ("filter_update", i32), ("filter_clip", f32),
        ("reward_mode", i32), ("ctrl_cost_weight", f32), ("contact_cost_weight", f32),
        ("gamma", f32), ("lambda_", f32), ("clip_param", f32), ("vf_clip_param", f32),
        ("vf_loss_coeff", f32), ("entropy_coeff", f32), ("lr", f32), ("grad_clip", f32),
        ("adam_beta1", f32), ("adam_beta2", f32), ("adam_eps", f32),
        ("vf_clip_mode", i32), ("sgd_minibatch_size", i32), ("num_sgd_iter", i32),
        ("act_negate", (i32 * 8) * MAX_AG), ("policy_filter", i32),
        ("leg_coupling", i32), ("gnn_layer", i32),
    ]


class DdrlEvalCfg(C.Structure):
    """ddrl_eval_cfg; the defaults are the reference's (evaluation/rollout_episodes.py:146, :152)."""
    _fields_ = [("episodes_per_env", i32), ("filter_update", i32), ("ctrl_roll", i32), ("reserved", i32),
                ("total_mass", C.c_double)]


TOTAL_MASS = 8.78710174560547   # mj_getTotalmass of the QuAntruped model (rollout_episodes.py:152)
EVAL_COLUMNS = ("reward", "steps", "distance", "power", "velocity", "cot")
EPISODE_COLUMNS = ("t", "env", "length", "total", "agent_0", "agent_1", "agent_2", "agent_3")

VP = C.c_void_p
_SIGS = {
    "ddrl_abi_version": ([], C.c_int),
    "ddrl_last_error": ([], C.c_char_p),
    "ddrl_ctx_create": ([C.POINTER(DdrlCfg), C.c_int, C.POINTER(VP)], C.c_int),
    "ddrl_ctx_destroy": ([VP], C.c_int),
    "ddrl_set_stream": ([VP, VP], C.c_int),
    "ddrl_synchronize": ([VP], C.c_int),
    "ddrl_param_count": ([VP, C.c_int, C.POINTER(C.c_int64)], C.c_int),
    "ddrl_record_layout": ([VP, C.c_int, C.POINTER(i32)], C.c_int),
    "ddrl_params_set": ([VP, C.c_int, VP, C.c_size_t], C.c_int),
    "ddrl_params_get": ([VP, C.c_int, VP, C.c_size_t], C.c_int),
    "ddrl_adam_set": ([VP, C.c_int, VP, VP, C.c_size_t, f32, f32], C.c_int),
    "ddrl_adam_get": ([VP, C.c_int, VP, VP, C.c_size_t, C.POINTER(f32), C.POINTER(f32)], C.c_int),
    "ddrl_filter_set": ([VP, C.c_double, VP, VP], C.c_int),
    "ddrl_filter_get": ([VP, C.POINTER(C.c_double), VP, VP], C.c_int),
    "ddrl_filter_delta_get": ([VP, C.POINTER(C.c_double), VP, VP], C.c_int),
    "ddrl_filter_delta_reset": ([VP], C.c_int),
    "ddrl_adv_sums_get": ([VP, C.c_int, VP], C.c_int),
    "ddrl_policy_filter_set": ([VP, C.c_int, C.c_double, VP, VP], C.c_int),
    "ddrl_policy_filter_get": ([VP, C.c_int, C.POINTER(C.c_double), VP, VP], C.c_int),
    "ddrl_policy_filter_delta_get": ([VP, C.c_int, C.POINTER(C.c_double), VP, VP], C.c_int),
    "ddrl_policy_filter_delta_reset": ([VP], C.c_int),
    "ddrl_observe": ([VP, VP], C.c_int),
    "ddrl_act": ([VP, C.c_int, VP, VP], C.c_int),
    "ddrl_reward": ([VP, C.c_int, VP, VP, VP, VP], C.c_int),
    "ddrl_bootstrap": ([VP], C.c_int),
    "ddrl_step_host": ([VP, C.c_int, VP, VP, VP], C.c_int),
    "ddrl_act_host": ([VP, C.c_int, VP, VP], C.c_int),
    "ddrl_rollout_fragment": ([VP, VP, VP, VP, VP, VP, VP], C.c_int),
    "ddrl_env_step_host": ([VP, C.c_int, VP, VP, VP, VP], C.c_int),
    "ddrl_gae": ([VP], C.c_int),
    "ddrl_ppo_update": ([VP, C.c_int, C.POINTER(VP), C.POINTER(VP), C.POINTER(f32), C.c_int], C.c_int),
    "ddrl_ppo_update_from": ([VP, C.c_int, C.POINTER(VP), C.POINTER(VP), C.POINTER(f32), C.c_int, C.c_int], C.c_int),
    "ddrl_ppo_stats": ([VP, C.c_int, VP, C.c_size_t], C.c_int),
    "ddrl_ppo_stats_range": ([VP, C.c_int, C.c_size_t, C.c_size_t, VP], C.c_int),
    "ddrl_ppo_grad": ([VP, C.c_int, VP, C.c_int, f32, VP, C.c_int], C.c_int),
    "ddrl_ppo_apply": ([VP, C.c_int, VP], C.c_int),
    "ddrl_comm_unique_id": ([VP, C.c_size_t], C.c_int),
    "ddrl_comm_init": ([VP, VP, C.c_int, C.c_int], C.c_int),
    "ddrl_comm_allreduce": ([VP, VP, C.c_size_t], C.c_int),
    "ddrl_ppo_update_ddp": ([VP, C.c_int, VP, VP, C.c_int, C.c_int, C.c_int, f32, f32], C.c_int),
    "ddrl_peer_alloc": ([VP, C.POINTER(VP), VP], C.c_int),
    "ddrl_peer_open": ([VP, VP, C.POINTER(VP)], C.c_int),
    "ddrl_peer_attach": ([VP, VP, C.c_int, C.c_int], C.c_int),
    "ddrl_ppo_update_peer": ([VP, C.c_int, VP, VP, C.c_int, C.c_int, f32, C.c_int], C.c_int),
    "ddrl_policy_forward": ([VP, C.c_int, VP, VP, C.c_int, VP, VP], C.c_int),
    "ddrl_gnn_one_launch": ([VP, C.POINTER(C.c_int)], C.c_int),
    "ddrl_device_buffers": ([VP, C.c_int, C.POINTER(VP), C.POINTER(VP), C.POINTER(VP), C.POINTER(VP)], C.c_int),
    "ddrl_records_get": ([VP, C.c_int, VP, C.c_size_t], C.c_int),
    "ddrl_records_set": ([VP, C.c_int, VP, C.c_size_t], C.c_int),
    "ddrl_adv_norm_get": ([VP, C.c_int, VP], C.c_int),
    "ddrl_adv_norm_set": ([VP, C.c_int, f32, f32], C.c_int),
    "ddrl_last_values_get": ([VP, C.c_int, VP, C.c_size_t], C.c_int),
    "ddrl_last_values_set": ([VP, C.c_int, VP, C.c_size_t], C.c_int),
    "ddrl_done_set": ([VP, VP, C.c_size_t], C.c_int),
    "ddrl_observe_range": ([VP, VP, C.c_int, C.c_int], C.c_int),
    "ddrl_act_range": ([VP, C.c_int, C.c_int, C.c_int, VP, VP], C.c_int),
    "ddrl_reward_range": ([VP, C.c_int, C.c_int, C.c_int, VP, VP, VP, VP], C.c_int),
    "ddrl_hostenv_last_error": ([], C.c_char_p),
    "ddrl_hostenv_create": ([C.c_int, C.c_int, C.c_int, C.c_uint64, f32, C.POINTER(VP)], C.c_int),
    "ddrl_hostenv_destroy": ([VP], C.c_int),
    "ddrl_hostenv_buffers": ([VP, C.POINTER(VP), C.POINTER(VP), C.POINTER(VP), C.POINTER(VP), C.POINTER(VP)],
                             C.c_int),
    "ddrl_hostenv_reset": ([VP], C.c_int),
    "ddrl_hostenv_step": ([VP, C.c_int, C.c_int], C.c_int),
    "ddrl_hostenv_threads": ([VP], C.c_int),
    "ddrl_hostenv_set_target_velocities": ([VP, C.POINTER(C.c_float), C.c_int], C.c_int),
    "ddrl_hostenv_target_velocities": ([VP, C.POINTER(C.c_float), C.c_int], C.c_int),
    "ddrl_hostenv_reset_state": ([VP], C.c_int),
    "ddrl_rollout_hostenv": ([VP, VP, C.c_int, VP, C.c_int], C.c_int),
    "ddrl_hostenv_kin": ([VP, C.POINTER(VP)], C.c_int),
    "ddrl_hostenv_set_time_limit": ([VP, C.c_int], C.c_int),
    "ddrl_hostenv_reset_episodes": ([VP], C.c_int),
    "ddrl_hostenv_state_get": ([VP, VP, C.c_size_t], C.c_int),
    "ddrl_hostenv_state_set": ([VP, VP, C.c_size_t], C.c_int),
    "ddrl_hostenv_set_terrain": ([VP, C.c_double, C.c_double, C.c_double, C.c_uint32], C.c_int),
    "ddrl_hostenv_terrain": ([VP, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                              C.POINTER(C.c_uint32)], C.c_int),
    "ddrl_hostenv_new_terrain": ([VP], C.c_int),
    "ddrl_hostenv_terrain_height": ([VP, VP, VP, C.c_int, VP], C.c_int),
    "ddrl_devenv_set_terrain": ([VP, C.c_double, C.c_double, C.c_double, C.c_uint32], C.c_int),
    "ddrl_devenv_terrain": ([VP, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                             C.POINTER(C.c_uint32)], C.c_int),
    "ddrl_devenv_new_terrain": ([VP], C.c_int),
    "ddrl_devenv_terrain_height": ([VP, VP, VP, C.c_int, VP], C.c_int),
    "ddrl_devenv_create": ([VP, C.c_uint64, f32, C.POINTER(VP)], C.c_int),
    "ddrl_devenv_destroy": ([VP], C.c_int),
    "ddrl_devenv_buffers": ([VP, C.POINTER(VP), C.POINTER(VP), C.POINTER(VP), C.POINTER(VP), C.POINTER(VP)],
                            C.c_int),
    "ddrl_devenv_reset": ([VP], C.c_int),
    "ddrl_devenv_reset_episodes": ([VP], C.c_int),
    "ddrl_devenv_reset_state": ([VP], C.c_int),
    "ddrl_devenv_set_time_limit": ([VP, C.c_int], C.c_int),
    "ddrl_devenv_set_target_velocities": ([VP, C.POINTER(C.c_float), C.c_int], C.c_int),
    "ddrl_devenv_target_velocities": ([VP, C.POINTER(C.c_float), C.c_int], C.c_int),
    "ddrl_devenv_set_env_target_velocities": ([VP, C.POINTER(C.c_float), C.c_int], C.c_int),
    "ddrl_devenv_step": ([VP, VP], C.c_int),
    "ddrl_devenv_state_get": ([VP, VP, C.c_size_t], C.c_int),
    "ddrl_devenv_state_set": ([VP, VP, C.c_size_t], C.c_int),
    "ddrl_rollout_devenv": ([VP, VP, VP, C.c_int], C.c_int),
    "ddrl_eval_devenv": ([VP, VP, VP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)], C.c_int),
    "ddrl_eval_begin": ([VP, C.POINTER(DdrlEvalCfg)], C.c_int),
    "ddrl_eval_act": ([VP, VP, VP, VP, C.POINTER(VP)], C.c_int),
    "ddrl_eval_step": ([VP, VP, VP, VP, VP, VP], C.c_int),
    "ddrl_eval_progress": ([VP, C.POINTER(C.c_int64), C.POINTER(C.c_int64)], C.c_int),
    "ddrl_eval_results": ([VP, VP, C.c_size_t], C.c_int),
    "ddrl_eval_end": ([VP], C.c_int),
    "ddrl_eval_hostenv": ([VP, VP, VP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)], C.c_int),
    "ddrl_eval_members_begin": ([VP, C.c_int], C.c_int),
    "ddrl_eval_member_load": ([VP, C.c_int], C.c_int),
    "ddrl_eval_member_filter_get": ([VP, C.c_int, VP, VP, VP], C.c_int),
    "ddrl_eval_sens_begin": ([VP, C.POINTER(VP)], C.c_int),
    "ddrl_eval_sens": ([VP, VP, C.POINTER(VP)], C.c_int),
    "ddrl_eval_sens_results": ([VP, C.c_int, VP, VP, C.POINTER(C.c_int64)], C.c_int),
    "ddrl_episodes_collect": ([VP, C.POINTER(C.c_int64)], C.c_int),
    "ddrl_episodes_rows": ([VP, VP, C.c_size_t], C.c_int),
    "ddrl_episodes_inflight": ([VP, VP, C.c_size_t], C.c_int),
    "ddrl_episodes_reset": ([VP], C.c_int),
    "ddrl_update_group_create": ([C.POINTER(VP), C.c_int, C.c_int, C.POINTER(VP)], C.c_int),
    "ddrl_update_group_run": ([VP, C.POINTER(VP), C.POINTER(VP), C.POINTER(f32), C.c_int], C.c_int),
    "ddrl_update_group_finish": ([VP], C.c_int),
    "ddrl_update_group_plan": ([C.c_int, C.c_int, C.c_int, C.POINTER(i32), C.POINTER(i32)], C.c_int),
    "ddrl_update_group_placement": ([VP, C.POINTER(i32), C.c_int], C.c_int),
    "ddrl_update_group_destroy": ([VP], C.c_int),
    "ddrl_update_group_stats_range": ([VP, C.c_size_t, C.c_size_t, VP], C.c_int),
    "ddrl_finish_group_create": ([C.POINTER(VP), C.c_int, C.POINTER(VP)], C.c_int),
    "ddrl_finish_group_run": ([VP, C.POINTER(C.c_int64)], C.c_int),
    "ddrl_finish_group_rows": ([VP, C.POINTER(VP), C.POINTER(C.c_int64)], C.c_int),
    "ddrl_finish_group_destroy": ([VP], C.c_int),
    "ddrl_rollout_group_create": ([C.POINTER(VP), C.POINTER(VP), C.c_int, C.POINTER(VP)], C.c_int),
    "ddrl_rollout_group_run": ([VP, C.POINTER(VP), C.c_int], C.c_int),
    "ddrl_rollout_group_destroy": ([VP], C.c_int),
    "ddrl_rng_seed": ([VP, C.c_int, C.c_uint64], C.c_int),
    "ddrl_rng_state_get": ([VP, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], C.c_int),
    "ddrl_rng_state_set": ([VP, C.c_int, C.c_uint64, C.c_uint64], C.c_int),
    "ddrl_noise_fill": ([VP, C.c_int, VP], C.c_int),
    "ddrl_schedule_fill": ([VP, C.c_int, C.POINTER(VP), C.POINTER(VP)], C.c_int),
    "ddrl_noise_fill_group": ([C.POINTER(VP), C.c_int, C.c_int, C.POINTER(VP)], C.c_int),
    "ddrl_schedule_fill_group": ([C.POINTER(VP), C.c_int, C.POINTER(VP), C.POINTER(VP)], C.c_int),
}

_lib = None


class DdrlError(RuntimeError):
    pass


def header_symbols(path=HEADER):
    """Function names declared in include/ddrl_hip.h."""
    txt = open(path).read()
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(ddrl_\w+)\s*\(", txt, re.M)))


ABI_VERSION = 4   # DDRL_ABI_VERSION of include/ddrl_hip.h (ddrl_cfg layout, record layout)
COMM_ID_BYTES = 128   # DDRL_COMM_ID_BYTES (sizeof ncclUniqueId)
PEER_HANDLE_BYTES = 64   # DDRL_PEER_HANDLE_BYTES (sizeof hipIpcMemHandle_t)
# DDRL_ENV_STATE_DOUBLES: the packed per-env state of both env planes, and its columns
ENV_STATE_DOUBLES = 41
ENV_STATE_COLUMNS = {"torso": slice(0, 10), "q": slice(10, 18), "qd": slice(18, 26), "qfrc": slice(26, 34),
                     "foot": slice(34, 38), "steps": 38, "episode": 39, "tv": 40}


def comm_unique_id():
    """A fresh RCCL unique id (rank 0 makes it, the caller hands it to the other ranks)."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _ck(load().ddrl_comm_unique_id(buf, COMM_ID_BYTES))
    return bytes(buf)


def load(path: str = LIB_PATH):
    """The HIP library.  DDRL_LIB names an alternative in-tree build of the same ABI (the
    diagnostic variants of ddrl_amd/build.py, e.g. libddrl_hip_atomic.so) for A/B timing."""
    global _lib
    if _lib is not None:
        return _lib
    if path == LIB_PATH and os.environ.get("DDRL_LIB"):
        path = os.path.join(HERE, os.path.basename(os.environ["DDRL_LIB"]))
    if not os.path.exists(path):
        raise DdrlError(f"{path} is missing: build it with `python -m ddrl_amd.build` "
                        "(the HIP library is the only compute path; there is no fallback)")
    # torch ships its own libamdhip64.so.7 (same soname as /opt/rocm's): import it first so
    # this library binds to the process's single HIP runtime instead of starting a second one
    import torch  # noqa: F401
    lib = C.CDLL(path)
    for name, (args, res) in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    if lib.ddrl_abi_version() != ABI_VERSION:
        raise DdrlError(f"{path} has ABI {lib.ddrl_abi_version()}, this binding expects {ABI_VERSION}: "
                        "rebuild with `python -m ddrl_amd.build`")
    _lib = lib
    return lib


def _ck(rc):
    if rc != 0:
        raise DdrlError(load().ddrl_last_error().decode())


def _ptr(x):
    """Device/host pointer of a torch tensor, numpy array, int or None."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"]
        return x.ctypes.data
    if hasattr(x, "data_ptr"):
        assert x.is_contiguous()
        return x.data_ptr()
    raise TypeError(type(x))


class Context:
    """One device + stream + rollout shard (a ddrl_ctx)."""

    def __init__(self, cfg: DdrlCfg, device: int = 0, stream: int | None = None):
        self.lib = load()
        self.cfg = cfg
        h = VP()
        _ck(self.lib.ddrl_ctx_create(C.byref(cfg), device, C.byref(h)))
        self.h = h
        self.device = device
        if stream is not None:
            self.set_stream(stream)
        self.n_params = []
        self.layout = []
        for p in range(cfg.n_policies):
            n = C.c_int64()
            _ck(self.lib.ddrl_param_count(h, p, C.byref(n)))
            self.n_params.append(int(n.value))
            lay = (i32 * 11)()
            _ck(self.lib.ddrl_record_layout(h, p, lay))
            self.layout.append(dict(zip(
                ["stride", "obs", "act", "logit", "logp", "vf", "adv", "vt", "rew", "C", "leg"], list(lay))))

    def close(self):
        if getattr(self, "h", None):
            self.lib.ddrl_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream: int):
        _ck(self.lib.ddrl_set_stream(self.h, stream))

    def synchronize(self):
        _ck(self.lib.ddrl_synchronize(self.h))

    # ---- state ----
    def params_set(self, pid, flat):
        a = np.ascontiguousarray(flat, np.float32)
        _ck(self.lib.ddrl_params_set(self.h, pid, a.ctypes.data, a.size))

    def params_get(self, pid):
        a = np.empty(self.n_params[pid], np.float32)
        _ck(self.lib.ddrl_params_get(self.h, pid, a.ctypes.data, a.size))
        return a

    def adam_set(self, pid, m, v, b1p, b2p):
        m = np.ascontiguousarray(m, np.float32)
        v = np.ascontiguousarray(v, np.float32)
        _ck(self.lib.ddrl_adam_set(self.h, pid, m.ctypes.data, v.ctypes.data, m.size, b1p, b2p))

    def adam_get(self, pid):
        n = self.n_params[pid]
        m, v = np.empty(n, np.float32), np.empty(n, np.float32)
        b1, b2 = f32(), f32()
        _ck(self.lib.ddrl_adam_get(self.h, pid, m.ctypes.data, v.ctypes.data, n, C.byref(b1), C.byref(b2)))
        return m, v, b1.value, b2.value

    def filter_set(self, n, M, S):
        M = np.ascontiguousarray(M, np.float64)
        S = np.ascontiguousarray(S, np.float64)
        _ck(self.lib.ddrl_filter_set(self.h, float(n), M.ctypes.data, S.ctypes.data))

    def filter_get(self):
        D = self.cfg.obs_full_dim
        n = C.c_double()
        M, S = np.empty(D), np.empty(D)
        _ck(self.lib.ddrl_filter_get(self.h, C.byref(n), M.ctypes.data, S.ctypes.data))
        return n.value, M, S

    def filter_delta_get(self):
        """Pushes since the last filter_delta_reset as (n, M, S)."""
        D = self.cfg.obs_full_dim
        n = C.c_double()
        M, S = np.empty(D), np.empty(D)
        _ck(self.lib.ddrl_filter_delta_get(self.h, C.byref(n), M.ctypes.data, S.ctypes.data))
        return n.value, M, S

    def filter_delta_reset(self):
        _ck(self.lib.ddrl_filter_delta_reset(self.h))

    def policy_filter_set(self, pid, n, M, S):
        M = np.ascontiguousarray(M, np.float64)
        S = np.ascontiguousarray(S, np.float64)
        _ck(self.lib.ddrl_policy_filter_set(self.h, pid, float(n), M.ctypes.data, S.ctypes.data))

    def policy_filter_get(self, pid, delta=False):
        d = self.cfg.obs_dim[pid]
        n = C.c_double()
        M, S = np.empty(d), np.empty(d)
        fn = self.lib.ddrl_policy_filter_delta_get if delta else self.lib.ddrl_policy_filter_get
        _ck(fn(self.h, pid, C.byref(n), M.ctypes.data, S.ctypes.data))
        return n.value, M, S

    def policy_filter_delta_reset(self):
        _ck(self.lib.ddrl_policy_filter_delta_reset(self.h))

    def adv_sums_get(self, pid):
        """fp64 (sum adv, sum adv^2, count) of the last gae() for policy pid."""
        a = np.empty(3, np.float64)
        _ck(self.lib.ddrl_adv_sums_get(self.h, pid, a.ctypes.data))
        return a

    def records_get(self, pid):
        lay = self.layout[pid]
        a = np.empty((self.cfg.frag_len * lay["C"], lay["stride"]), np.float32)
        _ck(self.lib.ddrl_records_get(self.h, pid, a.ctypes.data, a.size))
        return a

    def records_tensor(self, pid):
        """The policy's device record buffer [T * C][stride] as a torch tensor (no copy: a
        view over ddrl_device_buffers' pointer through __cuda_array_interface__)."""
        import torch
        rec, lv, par, an = VP(), VP(), VP(), VP()
        _ck(self.lib.ddrl_device_buffers(self.h, pid, C.byref(rec), C.byref(lv), C.byref(par), C.byref(an)))
        lay = self.layout[pid]
        shape = (self.cfg.frag_len * lay["C"], lay["stride"])

        class _View:
            __cuda_array_interface__ = {"shape": shape, "typestr": "<f4", "data": (rec.value, False),
                                        "version": 3, "strides": None}
        return torch.as_tensor(_View(), device=torch.device("cuda", self.device))

    def records_set(self, pid, rec):
        a = np.ascontiguousarray(rec, np.float32)
        _ck(self.lib.ddrl_records_set(self.h, pid, a.ctypes.data, a.size))

    def adv_norm_get(self, pid):
        a = np.empty(2, np.float32)
        _ck(self.lib.ddrl_adv_norm_get(self.h, pid, a.ctypes.data))
        return a

    def adv_norm_set(self, pid, mean, den):
        _ck(self.lib.ddrl_adv_norm_set(self.h, pid, mean, den))

    def last_values_get(self, pid):
        a = np.empty(self.layout[pid]["C"], np.float32)
        _ck(self.lib.ddrl_last_values_get(self.h, pid, a.ctypes.data, a.size))
        return a

    def last_values_set(self, pid, values):
        a = np.ascontiguousarray(values, np.float32)
        _ck(self.lib.ddrl_last_values_set(self.h, pid, a.ctypes.data, a.size))

    def done_set(self, done_tn):
        a = np.ascontiguousarray(done_tn, np.uint8)
        _ck(self.lib.ddrl_done_set(self.h, a.ctypes.data, a.size))

    # ---- rollout ----
    def observe(self, obs_dev):
        _ck(self.lib.ddrl_observe(self.h, _ptr(obs_dev)))

    def act(self, t, eps_dev, actions_dev):
        _ck(self.lib.ddrl_act(self.h, t, _ptr(eps_dev), _ptr(actions_dev)))

    def reward(self, t, fw_dev, cfrc_dev, actions_dev, done_dev=None):
        _ck(self.lib.ddrl_reward(self.h, t, _ptr(fw_dev), _ptr(cfrc_dev), _ptr(actions_dev), _ptr(done_dev)))

    def bootstrap(self):
        _ck(self.lib.ddrl_bootstrap(self.h))

    def step_host(self, t, obs_host, eps_host, actions_host):
        _ck(self.lib.ddrl_step_host(self.h, t, _ptr(obs_host), _ptr(eps_host), _ptr(actions_host)))

    def rollout_fragment(self, obs_dev, eps_dev, fw_dev, cfrc_dev, done_dev, actions_dev):
        _ck(self.lib.ddrl_rollout_fragment(self.h, _ptr(obs_dev), _ptr(eps_dev), _ptr(fw_dev), _ptr(cfrc_dev),
                                           _ptr(done_dev), _ptr(actions_dev)))

    def act_host(self, t, eps_host, actions_host):
        _ck(self.lib.ddrl_act_host(self.h, t, _ptr(eps_host), _ptr(actions_host)))

    def env_step_host(self, t, fw_host, cfrc_host, done_host, obs_next_host):
        _ck(self.lib.ddrl_env_step_host(self.h, t, _ptr(fw_host), _ptr(cfrc_host), _ptr(done_host),
                                        _ptr(obs_next_host)))

    def gae(self):
        _ck(self.lib.ddrl_gae(self.h))

    # ---- episode accounting of the training rollout ----
    def episodes_collect(self):
        """The episodes that finished in the fragment the context holds, float64 [n, 8] rows
        (EPISODE_COLUMNS) in ascending (t, env) order; agents the env does not have are NaN.
        Once per fragment, after its last reward; advances the in-flight state of every env."""
        n = C.c_int64()
        _ck(self.lib.ddrl_episodes_collect(self.h, C.byref(n)))
        a = np.empty((int(n.value), 8), np.float64)
        _ck(self.lib.ddrl_episodes_rows(self.h, a.ctypes.data, a.shape[0]))
        return a

    def episodes_inflight(self):
        """float64 [N, 6]: {total, agent_0 .. agent_3, length} of every env's running episode."""
        a = np.empty((self.cfg.n_envs, 6), np.float64)
        _ck(self.lib.ddrl_episodes_inflight(self.h, a.ctypes.data, a.shape[0]))
        return a

    def episodes_reset(self):
        """Forget the in-flight episodes."""
        _ck(self.lib.ddrl_episodes_reset(self.h))

    # ---- learner ----
    def ppo_update(self, mask, shuffles, perms, kl_coeffs, max_steps=-1, step0=0):
        """The fused minibatch SGD (ddrl_ppo_update); step0 > 0 resumes the schedule at that step
        (ddrl_ppo_update_from), bit-identical to the same steps of one uninterrupted launch."""
        P = self.cfg.n_policies
        sh = (VP * MAX_P)(*[_ptr(shuffles[p]) if shuffles[p] is not None else None for p in range(P)])
        pe = (VP * MAX_P)(*[_ptr(perms[p]) if perms[p] is not None else None for p in range(P)])
        kl = (f32 * MAX_P)(*[float(k) for k in kl_coeffs])
        if step0:
            _ck(self.lib.ddrl_ppo_update_from(self.h, mask, sh, pe, kl, step0, max_steps))
        else:
            _ck(self.lib.ddrl_ppo_update(self.h, mask, sh, pe, kl, max_steps))

    def ppo_stats(self, pid, n_steps, first=0):
        """Learner statistics rows [first, first + n_steps) of the last update (8 floats each)."""
        a = np.empty((n_steps, 8), np.float32)
        _ck(self.lib.ddrl_ppo_stats_range(self.h, pid, first, n_steps, a.ctypes.data))
        return a

    def ppo_grad(self, pid, rows_dev, n_rows, kl_coeff, grad_dev, stats_step=-1):
        _ck(self.lib.ddrl_ppo_grad(self.h, pid, _ptr(rows_dev), n_rows, kl_coeff, _ptr(grad_dev),
                                   stats_step))

    def ppo_apply(self, pid, grad_dev):
        _ck(self.lib.ddrl_ppo_apply(self.h, pid, _ptr(grad_dev)))

    def comm_init(self, unique_id, rank, nranks):
        """Join the RCCL communicator named by `unique_id` (bytes from comm_unique_id())."""
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        _ck(self.lib.ddrl_comm_init(self.h, buf, rank, nranks))

    def comm_allreduce(self, buf_dev):
        _ck(self.lib.ddrl_comm_allreduce(self.h, _ptr(buf_dev), buf_dev.numel()))

    def peer_alloc(self, export=False):
        """Rank 0: the shared outboxes of peer mode; (device pointer, IPC handle bytes or None)."""
        p = VP()
        h = (C.c_uint8 * PEER_HANDLE_BYTES)() if export else None
        _ck(self.lib.ddrl_peer_alloc(self.h, C.byref(p), h))
        return p.value, (bytes(h) if export else None)

    def peer_open(self, handle):
        """Rank 1 in another process: map rank 0's outboxes from its IPC handle."""
        buf = (C.c_uint8 * PEER_HANDLE_BYTES).from_buffer_copy(bytes(handle))
        p = VP()
        _ck(self.lib.ddrl_peer_open(self.h, buf, C.byref(p)))
        return p.value

    def peer_attach(self, gx_ptr, rank, nranks=2):
        _ck(self.lib.ddrl_peer_attach(self.h, VP(gx_ptr), rank, nranks))

    def ppo_update_peer(self, pid, shuffle_dev, perm_dev, kl_coeff, max_steps=-1):
        """One fused update with this rank's 64 rows of every minibatch (ddrl_ppo_update_peer);
        perm_dev: [n_epochs][nb] device int32, shuffle_dev: this rank's nb * 64 row indices."""
        E, nb = int(perm_dev.shape[0]), int(perm_dev.shape[1])
        _ck(self.lib.ddrl_ppo_update_peer(self.h, pid, _ptr(shuffle_dev), _ptr(perm_dev), E, nb, float(kl_coeff),
                                          max_steps))

    def gnn_one_launch(self):
        """True when the GraphNet minibatch step runs as one launch (reduction + clip + Adam in
        the gradient launch's tail), False for the three-launch step or an fcnet context."""
        on = C.c_int()
        _ck(self.lib.ddrl_gnn_one_launch(self.h, C.byref(on)))
        return bool(on.value)

    def ppo_update_ddp(self, pid, shuffle_dev, perms, rows_per_rank, kl_coeff, grad_scale):
        """The data-parallel minibatch loop in C++ (gradient -> RCCL all-reduce -> Adam per step)."""
        perms = np.ascontiguousarray(perms, np.int32)
        E, nb = perms.shape
        _ck(self.lib.ddrl_ppo_update_ddp(self.h, pid, _ptr(shuffle_dev), perms.ctypes.data, E, nb,
                                         rows_per_rank, kl_coeff, grad_scale))

    # ---- ranged rollout calls (env groups of a pipelined host env plane) ----
    def observe_range(self, obs_dev, e0, e1):
        _ck(self.lib.ddrl_observe_range(self.h, _ptr(obs_dev), e0, e1))

    def act_range(self, t, e0, e1, eps_dev, actions_dev):
        _ck(self.lib.ddrl_act_range(self.h, t, e0, e1, _ptr(eps_dev), _ptr(actions_dev)))

    def reward_range(self, t, e0, e1, fw_dev, cfrc_dev, actions_dev, done_dev=None):
        _ck(self.lib.ddrl_reward_range(self.h, t, e0, e1, _ptr(fw_dev), _ptr(cfrc_dev), _ptr(actions_dev),
                                       _ptr(done_dev)))

    def rollout_hostenv(self, env, eps_dev, groups=2, reset=False):
        """A fragment with the envs stepped on the host (HostEnv), pipelined over env groups."""
        _ck(self.lib.ddrl_rollout_hostenv(self.h, env.h, groups, _ptr(eps_dev), 1 if reset else 0))

    # ---- evaluation (whole episodes, N envs x E episodes each; fcnet models) ----
    def eval_begin(self, episodes_per_env, filter_update=False, ctrl_roll=2, total_mass=TOTAL_MASS):
        ec = DdrlEvalCfg(int(episodes_per_env), 1 if filter_update else 0, int(ctrl_roll), 0, float(total_mass))
        _ck(self.lib.ddrl_eval_begin(self.h, C.byref(ec)))
        self.eval_episodes = int(episodes_per_env)

    def eval_act(self, obs_dev, eps_dev, actions_dev, logits_out=None):
        """One fused launch from the raw observations to the env actions; eps_dev None takes the
        mean (explore=False).  logits_out: per policy a device buffer [C_p][2A] or None."""
        lo = None
        if logits_out is not None:
            lo = (VP * MAX_P)(*[_ptr(logits_out[p]) if p < len(logits_out) else None for p in range(MAX_P)])
        _ck(self.lib.ddrl_eval_act(self.h, _ptr(obs_dev), _ptr(eps_dev), _ptr(actions_dev), lo))

    def eval_step(self, fw_dev, cfrc_dev, actions_dev, kin_dev, done_dev):
        _ck(self.lib.ddrl_eval_step(self.h, _ptr(fw_dev), _ptr(cfrc_dev), _ptr(actions_dev), _ptr(kin_dev),
                                    _ptr(done_dev)))

    def eval_progress(self):
        """(rows written so far, envs that have filled their quota); synchronizes."""
        a, b = C.c_int64(), C.c_int64()
        _ck(self.lib.ddrl_eval_progress(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def eval_results(self):
        """float64 [N, E, 6] (EVAL_COLUMNS); rows of episodes that did not finish are NaN."""
        E = getattr(self, "eval_episodes", 0)
        a = np.empty((self.cfg.n_envs, E, 6), np.float64)
        _ck(self.lib.ddrl_eval_results(self.h, a.ctypes.data, self.cfg.n_envs * E))
        return a

    def eval_end(self):
        _ck(self.lib.ddrl_eval_end(self.h))

    def eval_hostenv(self, env, eps_dev=None, eps_steps=0, max_steps=1000, poll_every=25):
        """The whole evaluation over a HostEnv, loop in C++; returns the env steps taken."""
        n = C.c_int()
        _ck(self.lib.ddrl_eval_hostenv(self.h, env.h, _ptr(eps_dev), int(eps_steps), int(max_steps), int(poll_every),
                                       C.byref(n)))
        return int(n.value)

    def rollout_devenv(self, env, eps_dev, reset=False):
        """A fragment with the envs stepped on the device (DevEnv): one in-order chain of launches
        on the context's stream (a replayed HIP graph), no copies and no host wait."""
        _ck(self.lib.ddrl_rollout_devenv(self.h, env.h, _ptr(eps_dev), 1 if reset else 0))

    def eval_devenv(self, env, eps_dev=None, eps_steps=0, max_steps=1000, poll_every=25):
        """The whole evaluation over a DevEnv, loop in C++, the env's buffers read in place;
        returns the env steps taken."""
        n = C.c_int()
        _ck(self.lib.ddrl_eval_devenv(self.h, env.h, _ptr(eps_dev), int(eps_steps), int(max_steps), int(poll_every),
                                      C.byref(n)))
        return int(n.value)

    # ---- evaluation members: M parameter sets side by side, n_envs / M envs each ----
    def eval_members_begin(self, n_members):
        """After eval_begin: member m owns the envs [m n, (m + 1) n), n = n_envs / n_members, and
        eval_act runs every member on its own weights and filters.  All members start unloaded;
        eval_end (or the next eval_begin) ends the mode."""
        _ck(self.lib.ddrl_eval_members_begin(self.h, int(n_members)))

    def eval_member_load(self, member):
        """The context's current parameters, env-side filter and per-policy filters into the
        member's slot (device-to-device, stream-ordered): set them with params_set / filter_set /
        policy_filter_set first."""
        _ck(self.lib.ddrl_eval_member_load(self.h, int(member)))

    def eval_member_filter_get(self, member):
        """(n, M, S) of the member's env-side running stat; synchronizes."""
        D = self.cfg.obs_full_dim
        n = np.zeros(1, np.float64)
        M = np.zeros(D, np.float64)
        S = np.zeros(D, np.float64)
        _ck(self.lib.ddrl_eval_member_filter_get(self.h, int(member), n.ctypes.data, M.ctypes.data, S.ctypes.data))
        return float(n[0]), M, S

    # ---- input sensitivity of the evaluated policies (between eval_begin and eval_end) ----
    def eval_sens_begin(self, steps):
        """steps: per policy the perturbation h_f of each env-normalized input, obs_dim[p] finite
        values >= 0.  Clears the accumulators; eval_hostenv then runs eval_sens at every step."""
        if steps is None or len(steps) != self.cfg.n_policies:
            raise ValueError(f"steps: one array per policy ({self.cfg.n_policies})")
        arrs = []
        for p, s in enumerate(steps):
            a = np.ascontiguousarray(s, np.float64).reshape(-1)
            if a.size != self.cfg.obs_dim[p]:
                raise ValueError(f"steps[{p}]: {a.size} values, the policy takes {self.cfg.obs_dim[p]}")
            arrs.append(a)
        tab = (VP * MAX_P)(*[arrs[p].ctypes.data if p < len(arrs) else None for p in range(MAX_P)])
        _ck(self.lib.ddrl_eval_sens_begin(self.h, tab))

    def eval_sens(self, obs_dev, means_out=None):
        """After eval_act of the same observations, before eval_step.  means_out: per policy a
        device buffer [C_p][2 d][A] (float32) or None."""
        mo = None
        if means_out is not None:
            mo = (VP * MAX_P)(*[_ptr(means_out[p]) if p < len(means_out) else None for p in range(MAX_P)])
        _ck(self.lib.ddrl_eval_sens(self.h, _ptr(obs_dev), mo))

    def eval_sens_results(self, pid):
        """(grads [d, A], grads_abs [d, A], rows) of policy pid; synchronizes."""
        d, A = (self.cfg.obs_dim[pid], self.cfg.act_dim) if 0 <= pid < self.cfg.n_policies else (1, 1)
        g, ga, rows = np.zeros((d, A)), np.zeros((d, A)), C.c_int64()
        _ck(self.lib.ddrl_eval_sens_results(self.h, int(pid), g.ctypes.data, ga.ctypes.data, C.byref(rows)))
        return g, ga, int(rows.value)

    def policy_forward(self, pid, obs_dev, n, logits_dev, values_dev, node_dev=None):
        _ck(self.lib.ddrl_policy_forward(self.h, pid, _ptr(obs_dev), _ptr(node_dev), n,
                                         _ptr(logits_dev), _ptr(values_dev)))

    # ---- device randomness: noise and schedules drawn by the counter-based generator ----
    def rng_seed(self, stream, seed):
        """Seed the RNG_NOISE or RNG_SCHEDULE stream (any Python int, taken modulo 2^64); its
        position restarts at 0."""
        _ck(self.lib.ddrl_rng_seed(self.h, int(stream), int(seed) & _U64))

    def rng_state(self, stream):
        """(seed, position) of the stream: all of its state."""
        s, pos = C.c_uint64(), C.c_uint64()
        _ck(self.lib.ddrl_rng_state_get(self.h, int(stream), C.byref(s), C.byref(pos)))
        return int(s.value), int(pos.value)

    def rng_state_set(self, stream, seed, position):
        _ck(self.lib.ddrl_rng_state_set(self.h, int(stream), int(seed) & _U64, int(position) & _U64))

    def noise_fill(self, n_steps, eps_dev):
        """eps_dev [n_steps, N, n_agents, A] float32 <- the next n_steps steps of the noise stream."""
        _ck(self.lib.ddrl_noise_fill(self.h, int(n_steps), _ptr(eps_dev)))

    def schedule_alloc(self, device=None):
        """Persistent device arrays for schedule_fill: (shuffles, perms), per policy int32 [R_p] and
        [num_sgd_iter, nb_p], the shapes ppo_update takes."""
        import torch
        dev = torch.device("cuda", self.device) if device is None else device
        mb, T, E = self.cfg.sgd_minibatch_size, self.cfg.frag_len, self.cfg.num_sgd_iter
        R = [T * self.layout[p]["C"] for p in range(self.cfg.n_policies)]
        return ([torch.empty(r, dtype=torch.int32, device=dev) for r in R],
                [torch.empty((E, max(1, r // mb)), dtype=torch.int32, device=dev) for r in R])

    def schedule_fill(self, shuffles, perms, mask=None):
        """The next draw of the schedule stream into the policies of `mask` (default: all)."""
        P = self.cfg.n_policies
        mask = (1 << P) - 1 if mask is None else int(mask)
        sh = (VP * MAX_P)(*[_ptr(shuffles[p]) if p < len(shuffles) else None for p in range(MAX_P)])
        pe = (VP * MAX_P)(*[_ptr(perms[p]) if p < len(perms) else None for p in range(MAX_P)])
        _ck(self.lib.ddrl_schedule_fill(self.h, mask, sh, pe))


def _terrain_args(lo, hi, generation, current_generation):
    """(lo, hi, generation) of a set_terrain call: hi None is lo, generation None the current one."""
    lo = float(lo)
    hi = lo if hi is None else float(hi)
    gen = int(current_generation() if generation is None else generation)
    if not 0 <= gen <= 0xFFFFFFFF:
        raise DdrlError("set_terrain: generation must fit an unsigned 32-bit integer")
    return lo, hi, gen


def _terrain_points(env_index, xy, n_envs):
    """(int32 [n], float64 [n][2]) of a terrain_height call, the env indices checked."""
    pts = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    idx = np.array(np.broadcast_to(np.asarray(env_index, np.int32), (pts.shape[0],)))   # a writable copy
    if idx.size and (idx.min() < 0 or idx.max() >= n_envs):
        raise DdrlError(f"terrain_height: env index out of range [0, {n_envs})")
    return idx, pts


def noise_fill_group(contexts, n_steps, eps_devs):
    """Context.noise_fill for every member in one launch (ddrl_noise_fill_group): eps_devs[m] is
    member m's buffer; every member's noise stream advances by n_steps."""
    cs, eps = list(contexts), list(eps_devs)
    if len(cs) != len(eps):
        raise DdrlError(f"noise fill group: {len(cs)} contexts and {len(eps)} noise buffers")
    n = len(cs)
    _ck(load().ddrl_noise_fill_group((VP * max(1, n))(*[c.h for c in cs]), n, int(n_steps),
                                     (VP * max(1, n))(*[_ptr(x) for x in eps])))


def schedule_fill_group(contexts, shuffles, perms):
    """Context.schedule_fill of all policies for every member in one launch
    (ddrl_schedule_fill_group): shuffles / perms hold one list per member, one entry per policy."""
    cs = list(contexts)
    P = cs[0].cfg.n_policies if cs else 0
    flat = lambda xs: [x for member in xs for x in list(member)[:P]]
    sh, pe = flat(shuffles), flat(perms)
    n = len(cs) * P
    if not (len(sh) == len(pe) == n):
        raise DdrlError(f"schedule fill group: {n} (member, policy) entries expected")
    _ck(load().ddrl_schedule_fill_group((VP * max(1, len(cs)))(*[c.h for c in cs]), len(cs),
                                        (VP * max(1, n))(*[_ptr(x) for x in sh]), (VP * max(1, n))(*[_ptr(x) for x in pe])))


def update_group_grid(n_chains):
    """Blocks of a group launch of n_chains chains: 32 per full group row of 8, 24 + chains in the last."""
    rows = (n_chains + 7) // 8
    return 32 * (rows - 1) + 24 + (n_chains - 8 * (rows - 1))


def update_group_plan(n_members, n_policies, max_chains):
    """ddrl_update_group_plan (pure host, no GPU): (launch_of_member[M], first_block_of_chain[M, P]) for
    launches of at most max_chains chains; chain (m, p) runs on blocks first_block + 8 j, j = 0 .. 3,
    of its launch's grid."""
    lom = (i32 * max(1, n_members))()
    fb = (i32 * max(1, n_members * n_policies))()
    _ck(load().ddrl_update_group_plan(n_members, n_policies, max_chains, lom, fb))
    return (np.array(lom[:n_members], np.int32),
            np.array(fb[:n_members * n_policies], np.int32).reshape(n_members, n_policies))


class UpdateGroup:
    """The fused updates of several same-shaped contexts in one launch (a ddrl_update_group): every
    member's chains bit-identical to its own Context.ppo_update.  Close the group before its members."""

    def __init__(self, contexts, max_chains_per_launch=0):
        self.lib = load()
        self.contexts = list(contexts)
        self.P = self.contexts[0].cfg.n_policies if self.contexts else 0
        hs = (VP * max(1, len(self.contexts)))(*[c.h for c in self.contexts])
        h = VP()
        _ck(self.lib.ddrl_update_group_create(hs, len(self.contexts), max_chains_per_launch, C.byref(h)))
        self.h = h

    def _h(self):
        if not getattr(self, "h", None):
            raise DdrlError("update group: used after close")
        return self.h

    def run(self, shuffles, perms, kl_coeffs, max_steps=-1):
        """shuffles / perms / kl_coeffs: one list per member, one entry per policy; asynchronous."""
        h = self._h()
        n = len(self.contexts) * self.P
        flat = lambda xs: [x for member in xs for x in list(member)[:self.P]]
        sh, pe, kl = flat(shuffles), flat(perms), flat(kl_coeffs)
        if not (len(sh) == len(pe) == len(kl) == n):
            raise DdrlError(f"update group: {n} (member, policy) entries expected")
        self._keep = (sh, pe)   # the device schedules stay alive until the run is finished
        _ck(self.lib.ddrl_update_group_run(h, (VP * n)(*[_ptr(x) for x in sh]), (VP * n)(*[_ptr(x) for x in pe]),
                                           (f32 * n)(*[float(k) for k in kl]), max_steps))

    def finish(self):
        """Synchronize and check; on failure every member is as before the run and DdrlError is raised."""
        try:
            _ck(self.lib.ddrl_update_group_finish(self._h()))
        finally:
            self._keep = None

    def stats_range(self, first, n_steps):
        """Context.ppo_stats(p, n_steps, first) of every member and policy after a finished run,
        float32 [M, P, n_steps, 8], with one synchronize for the group."""
        a = np.empty((len(self.contexts), self.P, int(n_steps), 8), np.float32)
        _ck(self.lib.ddrl_update_group_stats_range(self._h(), int(first), int(n_steps), a.ctypes.data))
        return a

    def placement(self):
        """XCC id of every block of the last finished run: the launches' grids in launch order, one flat
        array (update_group_plan and update_group_grid give each launch's share)."""
        n = 32 * max(1, len(self.contexts) * self.P)   # a launch of n chains has at most 32 n blocks
        x = (i32 * n)()
        _ck(self.lib.ddrl_update_group_placement(self._h(), x, n))
        a = np.array(x[:], np.int32)
        return a[:int((a >= 0).sum())]

    def close(self):
        if getattr(self, "h", None):
            self.lib.ddrl_update_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RolloutGroup:
    """The device-plane fragments of several same-shaped contexts as one chain of launches (a
    ddrl_rollout_group): member m = (contexts[m], envs[m]), bit-identical to its own
    Context.rollout_devenv.  Close the group before its members and their envs."""

    def __init__(self, contexts, envs):
        self.lib = load()
        self.contexts, self.envs = list(contexts), list(envs)
        if len(self.contexts) != len(self.envs):
            raise DdrlError(f"rollout group: {len(self.contexts)} contexts and {len(self.envs)} device envs")
        n = len(self.contexts)
        cs = (VP * max(1, n))(*[c.h for c in self.contexts])
        es = (VP * max(1, n))(*[e.h for e in self.envs])
        h = VP()
        _ck(self.lib.ddrl_rollout_group_create(cs, es, n, C.byref(h)))
        self.h = h

    def run(self, eps_devs, reset=False):
        """eps_devs: one [T, N, n_agents, A] float32 device tensor per member; asynchronous, on the
        members' stream."""
        if not getattr(self, "h", None):
            raise DdrlError("rollout group: used after close")
        eps = list(eps_devs)
        if len(eps) != len(self.contexts):
            raise DdrlError(f"rollout group: {len(self.contexts)} noise buffers expected")
        _ck(self.lib.ddrl_rollout_group_run(self.h, (VP * max(1, len(eps)))(*[_ptr(x) for x in eps]),
                                            1 if reset else 0))

    def close(self):
        if getattr(self, "h", None):
            self.lib.ddrl_rollout_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FinishGroup:
    """Context.gae + Context.episodes_collect of several same-shaped contexts as one chain of launches
    (a ddrl_finish_group), every member left bit-identical to its own calls.  Any env plane and model
    kind: only the records are read.  Close the group before its members."""

    def __init__(self, contexts):
        self.lib = load()
        self.contexts = list(contexts)
        n = len(self.contexts)
        h = VP()
        _ck(self.lib.ddrl_finish_group_create((VP * max(1, n))(*[c.h for c in self.contexts]), n, C.byref(h)))
        self.h = h

    def run(self):
        """One float64 [n_m, 8] array of episode rows (EPISODE_COLUMNS) per member; synchronizes."""
        if not getattr(self, "h", None):
            raise DdrlError("finish group: used after close")
        n = len(self.contexts)
        counts = (C.c_int64 * n)()
        _ck(self.lib.ddrl_finish_group_run(self.h, counts))
        rows = [np.empty((int(k), 8), np.float64) for k in counts]
        _ck(self.lib.ddrl_finish_group_rows(self.h, (VP * n)(*[a.ctypes.data for a in rows]), counts))
        return rows

    def close(self):
        if getattr(self, "h", None):
            self.lib.ddrl_finish_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostEnv:
    """The host env plane (hostenv.cpp): N QuAntruped stand-in envs stepped by a pool of host
    threads into pinned buffers, exposed here as numpy views (obs [N][D], act [N][8], fw [N],
    cfrc [N][14][6], done [N])."""

    def __init__(self, n_envs, obs_dim=43, n_threads=1, seed=0, target_velocity=0.0):
        """target_velocity: one value, or a list every env draws its episode's velocity from on
        each reset (the adaptor's random.choice, quantruped_adaptor_multi_environment.py:50, 216)."""
        self.lib = load()
        h = VP()
        tvs = [float(v) for v in (target_velocity if np.ndim(target_velocity) else [target_velocity])]
        if self.lib.ddrl_hostenv_create(n_envs, obs_dim, n_threads, seed, tvs[0], C.byref(h)) != 0:
            raise DdrlError(self.lib.ddrl_hostenv_last_error().decode())
        if len(tvs) > 1:
            arr = (C.c_float * len(tvs))(*tvs)
            if self.lib.ddrl_hostenv_set_target_velocities(h, arr, len(tvs)) != 0:
                err = self.lib.ddrl_hostenv_last_error().decode()
                self.lib.ddrl_hostenv_destroy(h)
                raise DdrlError(err)
        self.h, self.n, self.obs_dim = h, n_envs, obs_dim
        ptrs = [VP() for _ in range(5)]
        self._ck(self.lib.ddrl_hostenv_buffers(h, *[C.byref(p) for p in ptrs]))
        view = lambda p, ct, shape: np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=shape)
        self.obs = view(ptrs[0], C.c_float, (n_envs, obs_dim))
        self.act = view(ptrs[1], C.c_float, (n_envs, 8))
        self.fw = view(ptrs[2], C.c_float, (n_envs,))
        self.cfrc = view(ptrs[3], C.c_float, (n_envs, 14, 6))
        self.done = view(ptrs[4], C.c_uint8, (n_envs,))
        self.threads = self.lib.ddrl_hostenv_threads(h)
        kp = VP()
        self._ck(self.lib.ddrl_hostenv_kin(h, C.byref(kp)))
        self.kin = view(kp, C.c_float, (n_envs, 9))   # {dx, joint qvel[8]} of the step, pre-reset

    def _ck(self, rc):
        if rc != 0:
            raise DdrlError(self.lib.ddrl_hostenv_last_error().decode())

    def _live(self):
        if not getattr(self, "h", None):
            raise DdrlError("host env plane is closed")

    def reset(self):
        """Reset every env; returns a COPY of the observations (self.obs is the live pinned
        buffer that the next step() overwrites in place)."""
        self._live()
        self._ck(self.lib.ddrl_hostenv_reset(self.h))
        return self.obs.copy()

    def step(self, e0=0, e1=None):
        """Step the envs [e0, e1) with the actions in self.act (written by the caller)."""
        self._live()
        self._ck(self.lib.ddrl_hostenv_step(self.h, e0, self.n if e1 is None else e1))

    def reset_state(self):
        """update_environment_after_epoch's env.reset(): every env's state and TimeLimit count
        restart; target velocities, done flags and self.obs are left as they are."""
        self._live()
        self._ck(self.lib.ddrl_hostenv_reset_state(self.h))

    def set_time_limit(self, steps):
        """The TimeLimit of every env (default 1000): an episode ends after `steps` steps."""
        self._live()
        self._ck(self.lib.ddrl_hostenv_set_time_limit(self.h, int(steps)))

    def reset_episodes(self):
        """Every env starts a fresh episode at step 0 (reset() staggers the episode phases);
        returns a copy of the observations."""
        self._live()
        self._ck(self.lib.ddrl_hostenv_reset_episodes(self.h))
        return self.obs.copy()

    def state(self):
        """The packed fp64 state of every env, [N, ENV_STATE_DOUBLES] (ENV_STATE_COLUMNS)."""
        self._live()
        a = np.empty((self.n, ENV_STATE_DOUBLES), np.float64)
        self._ck(self.lib.ddrl_hostenv_state_get(self.h, a.ctypes.data, a.size))
        return a

    def set_state(self, state):
        """Replace every env's state (the output buffers keep their contents until the next step)."""
        self._live()
        a = np.ascontiguousarray(state, np.float64)
        self._ck(self.lib.ddrl_hostenv_state_set(self.h, a.ctypes.data, a.size))

    def set_terrain(self, lo, hi=None, bump_scale=2.0, generation=None):
        """Uneven ground (the reference's hf_smoothness): every env draws its smoothness from
        [lo, hi] per terrain generation; hi None is the fixed smoothness lo.  1 is flat (the
        default), 0 the roughest.  bump_scale: metres between bumps (hf_bump_scale).  generation
        None keeps the current one."""
        self._live()
        lo, hi, gen = _terrain_args(lo, hi, generation, lambda: self.terrain["generation"])
        self._ck(self.lib.ddrl_hostenv_set_terrain(self.h, lo, hi, float(bump_scale), gen))

    @property
    def terrain(self):
        """{"lo", "hi", "bump_scale", "generation"} as set_terrain / new_terrain left them."""
        self._live()
        lo, hi, bs, gen = C.c_double(), C.c_double(), C.c_double(), C.c_uint32()
        self._ck(self.lib.ddrl_hostenv_terrain(self.h, C.byref(lo), C.byref(hi), C.byref(bs), C.byref(gen)))
        return {"lo": lo.value, "hi": hi.value, "bump_scale": bs.value, "generation": gen.value}

    def new_terrain(self):
        """create_new_random_hfield: the next terrain generation, new ground for every env."""
        self._live()
        self._ck(self.lib.ddrl_hostenv_new_terrain(self.h))

    def terrain_height(self, env_index, xy):
        """The ground height of env env_index[i]'s current field at xy[i] = (x, y); [n] float64."""
        self._live()
        idx, pts = _terrain_points(env_index, xy, self.n)
        out = np.empty(idx.size, np.float64)
        self._ck(self.lib.ddrl_hostenv_terrain_height(self.h, idx.ctypes.data, pts.ctypes.data, idx.size,
                                                      out.ctypes.data))
        return out

    @property
    def target_velocities(self):
        """Each env's current target velocity (the draw of its current episode)."""
        self._live()
        out = np.zeros(self.n, np.float32)
        self._ck(self.lib.ddrl_hostenv_target_velocities(self.h, out.ctypes.data_as(C.POINTER(C.c_float)), self.n))
        return out

    def close(self):
        """Free the pinned buffers.  The numpy views over them are dropped first (set to None),
        so no attribute of this object can read freed memory afterwards; copies made by the
        caller stay valid."""
        if getattr(self, "h", None):
            self.obs = self.act = self.fw = self.cfrc = self.done = self.kin = None
            self.lib.ddrl_hostenv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DevEnv:
    """The device env plane (devenv.hip): the context's N stand-in envs stepped by a HIP kernel on
    the context's stream.  obs [N][D], fw [N], cfrc [N][14][6], kin [N][9] and done [N] are torch
    CUDA tensors over the library's memory (no copy); a step rewrites them in place."""

    def __init__(self, ctx: Context, seed=0, target_velocity=0.0):
        """target_velocity: one value, or the list every env draws its episode's velocity from."""
        import torch
        self.lib = load()
        self.ctx = ctx   # keeps the context alive; close() the env before the context
        h = VP()
        tvs = [float(v) for v in (target_velocity if np.ndim(target_velocity) else [target_velocity])]
        _ck(self.lib.ddrl_devenv_create(ctx.h, seed, tvs[0], C.byref(h)))
        self.h, self.n, self.obs_dim = h, ctx.cfg.n_envs, ctx.cfg.obs_full_dim
        if len(tvs) > 1:
            try:
                self.set_target_velocities(tvs)
            except DdrlError:
                self.lib.ddrl_devenv_destroy(h)
                self.h = None
                raise
        ptrs = [VP() for _ in range(5)]
        _ck(self.lib.ddrl_devenv_buffers(h, *[C.byref(p) for p in ptrs]))
        dev = torch.device("cuda", ctx.device)

        def view(p, typestr, shape):
            class _View:
                __cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (p.value, False),
                                            "version": 3, "strides": None}
            return torch.as_tensor(_View(), device=dev)
        n, D = self.n, self.obs_dim
        self.obs = view(ptrs[0], "<f4", (n, D))
        self.fw = view(ptrs[1], "<f4", (n,))
        self.cfrc = view(ptrs[2], "<f4", (n, 14, 6))
        self.kin = view(ptrs[3], "<f4", (n, 9))
        self.done = view(ptrs[4], "|u1", (n,))

    def _live(self):
        if not getattr(self, "h", None):
            raise DdrlError("device env plane is closed")

    def reset(self):
        """Reset every env (staggered episode phases); returns self.obs, the live buffer."""
        self._live()
        _ck(self.lib.ddrl_devenv_reset(self.h))
        return self.obs

    def reset_episodes(self):
        """Every env starts a fresh episode at step 0; returns self.obs."""
        self._live()
        _ck(self.lib.ddrl_devenv_reset_episodes(self.h))
        return self.obs

    def reset_state(self):
        """update_environment_after_epoch's env.reset(): state and TimeLimit count restart; target
        velocities, done flags and self.obs stay."""
        self._live()
        _ck(self.lib.ddrl_devenv_reset_state(self.h))

    def set_time_limit(self, steps):
        self._live()
        _ck(self.lib.ddrl_devenv_set_time_limit(self.h, int(steps)))

    def set_target_velocities(self, tvs):
        self._live()
        tvs = [float(v) for v in tvs]
        _ck(self.lib.ddrl_devenv_set_target_velocities(self.h, (C.c_float * len(tvs))(*tvs), len(tvs)))

    def set_env_target_velocities(self, tvs):
        """A fixed target velocity per env (n_envs values) at every reset and episode restart, or
        None to go back to drawing from the list."""
        self._live()
        if tvs is None:
            _ck(self.lib.ddrl_devenv_set_env_target_velocities(self.h, None, 0))
            return
        tvs = [float(v) for v in np.asarray(tvs).reshape(-1)]
        _ck(self.lib.ddrl_devenv_set_env_target_velocities(self.h, (C.c_float * len(tvs))(*tvs), len(tvs)))

    def set_terrain(self, lo, hi=None, bump_scale=2.0, generation=None):
        """HostEnv.set_terrain for the device plane: holds for the launches issued after it."""
        self._live()
        lo, hi, gen = _terrain_args(lo, hi, generation, lambda: self.terrain["generation"])
        _ck(self.lib.ddrl_devenv_set_terrain(self.h, lo, hi, float(bump_scale), gen))

    @property
    def terrain(self):
        """{"lo", "hi", "bump_scale", "generation"} as set_terrain / new_terrain left them."""
        self._live()
        lo, hi, bs, gen = C.c_double(), C.c_double(), C.c_double(), C.c_uint32()
        _ck(self.lib.ddrl_devenv_terrain(self.h, C.byref(lo), C.byref(hi), C.byref(bs), C.byref(gen)))
        return {"lo": lo.value, "hi": hi.value, "bump_scale": bs.value, "generation": gen.value}

    def new_terrain(self):
        """create_new_random_hfield: the next terrain generation, new ground for every env."""
        self._live()
        _ck(self.lib.ddrl_devenv_new_terrain(self.h))

    def terrain_height(self, env_index, xy):
        """The ground height of env env_index[i]'s current field at xy[i], computed by a kernel
        on the context's stream; [n] float64 on the host.  Synchronizes."""
        import torch
        self._live()
        idx, pts = _terrain_points(env_index, xy, self.n)
        dev = torch.device("cuda", self.ctx.device)
        idx_d, pts_d = torch.from_numpy(idx).to(dev), torch.from_numpy(pts).to(dev)
        out = torch.empty(idx.size, dtype=torch.float64, device=dev)
        _ck(self.lib.ddrl_devenv_terrain_height(self.h, _ptr(idx_d), _ptr(pts_d), idx.size, _ptr(out)))
        self.ctx.synchronize()
        return out.cpu().numpy()

    @property
    def target_velocities(self):
        """Each env's current target velocity; synchronizes."""
        self._live()
        out = np.zeros(self.n, np.float32)
        _ck(self.lib.ddrl_devenv_target_velocities(self.h, out.ctypes.data_as(C.POINTER(C.c_float)), self.n))
        return out

    def step(self, actions_dev):
        """One launch on the context's stream: actions_dev [N][8] float32 in device memory."""
        self._live()
        _ck(self.lib.ddrl_devenv_step(self.h, _ptr(actions_dev)))

    def state(self):
        """The packed fp64 state of every env, [N, ENV_STATE_DOUBLES]; synchronizes."""
        self._live()
        a = np.empty((self.n, ENV_STATE_DOUBLES), np.float64)
        _ck(self.lib.ddrl_devenv_state_get(self.h, a.ctypes.data, a.size))
        return a

    def set_state(self, state):
        self._live()
        a = np.ascontiguousarray(state, np.float64)
        _ck(self.lib.ddrl_devenv_state_set(self.h, a.ctypes.data, a.size))

    def close(self):
        """Free the device buffers; the tensors over them are dropped first."""
        if getattr(self, "h", None):
            self.obs = self.fw = self.cfrc = self.kin = self.done = None
            self.lib.ddrl_devenv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
