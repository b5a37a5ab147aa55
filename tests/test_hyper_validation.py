"""CPU checks of the hyperparameters ddrl_ctx_create refuses: a NaN in any of them, and a
grad_clip <= 0 (the clip scale grad_clip * min(1 / norm, 1 / grad_clip) is then NaN or 0 * inf,
NaN in every parameter after the first step).  validate() runs before any device call, so the
refusals, and that the legal edge values pass it, show without a GPU: there the create of a legal
configuration still fails, on its first device call and with another message."""
import ctypes

import pytest

from ddrl_amd import build, native
from ddrl_amd.spec import make_cfg

ENV = "QuantrupedMultiEnv_Local"
FIELDS = ["gamma", "lambda_", "clip_param", "vf_clip_param", "vf_loss_coeff", "entropy_coeff", "lr", "grad_clip",
          "adam_beta1", "adam_beta2", "adam_eps"]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return native.load()


def _create(lib, config=None, **fields):
    """ddrl_ctx_create with `fields` set on the ddrl_cfg -> (rc, ddrl_last_error())."""
    cfg, _ = make_cfg(ENV, 4, 2, config)
    for name, value in fields.items():
        assert hasattr(cfg, name), name
        setattr(cfg, name, value)
    h = ctypes.c_void_p()
    rc = lib.ddrl_ctx_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    err = lib.ddrl_last_error() if rc else b""
    if rc == 0:
        lib.ddrl_ctx_destroy(h)
    return rc, err


def _refused_hyper(err):
    return b"NaN" in err or b"grad_clip" in err


@pytest.mark.parametrize("field", FIELDS)
def test_nan_hyperparameter_is_refused_by_name(lib, field):
    rc, err = _create(lib, **{field: float("nan")})
    assert rc != 0 and field.encode() in err and b"NaN" in err, err
    # the message names this field and no other
    assert not any(f.encode() in err for f in FIELDS if f != field and f not in field), err


@pytest.mark.parametrize("clip", [0.0, -0.5, -1e30, float("-inf")])
def test_non_positive_grad_clip_is_refused(lib, clip):
    rc, err = _create(lib, grad_clip=clip)
    assert rc != 0 and b"grad_clip" in err, err


def test_config_keys_reach_the_refusal(lib):
    """The same through make_cfg's RLlib-style keys."""
    rc, err = _create(lib, {"grad_clip": 0})
    assert rc != 0 and b"grad_clip" in err, err
    rc, err = _create(lib, {"entropy_coeff": float("nan")})
    assert rc != 0 and b"entropy_coeff" in err, err


@pytest.mark.parametrize("config", [None, {"lr": 0.0}, {"grad_clip": None}, {"grad_clip": 1e30}, {"grad_clip": 1e-6},
                                    {"grad_clip": 40.0, "entropy_coeff": -0.005, "vf_loss_coeff": 0.0},
                                    {"vf_clip_mode": "squared", "vf_clip_param": 1.0, "clip_param": 0.3}])
def test_legal_edge_values_pass_validation(lib, config):
    cfg, _ = make_cfg(ENV, 4, 2, config)
    if config and config.get("grad_clip", 0.5) is None:
        assert cfg.grad_clip == pytest.approx(1e30)      # grad_clip None: no clipping
    rc, err = _create(lib, config)
    assert not _refused_hyper(err), err
