"""CPU checks of the finish group's C-ABI boundary: the header declares the five new functions,
native.py binds each with the header's argument count, the library exports them, and the calls
that need no device refuse null arguments with a message."""
import ctypes
import re

import pytest

from ddrl_amd import build, native

NEW = ("ddrl_finish_group_create", "ddrl_finish_group_run", "ddrl_finish_group_rows",
       "ddrl_finish_group_destroy", "ddrl_update_group_stats_range")


def _header_arg_counts():
    txt = re.sub(r"/\*.*?\*/", "", open(native.HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"^\s*int\s+(ddrl_\w+)\s*\(([^)]*)\)\s*;", txt, re.M):
        out[name] = 0 if args.strip() in ("", "void") else args.count(",") + 1
    return out


@pytest.fixture(scope="module")
def lib():
    build.build()
    return native.load()


def test_header_declares_the_new_functions():
    syms = native.header_symbols()
    for name in NEW:
        assert name in syms, name
    assert "typedef struct ddrl_finish_group ddrl_finish_group;" in open(native.HEADER).read()


@pytest.mark.parametrize("name", NEW)
def test_binding_matches_the_header(lib, name):
    counts = _header_arg_counts()
    assert name in native._SIGS, name
    args, res = native._SIGS[name]
    assert len(args) == counts[name], (name, len(args), counts[name])
    assert res is ctypes.c_int
    assert hasattr(lib, name)


def test_python_wrappers_exist():
    assert callable(native.FinishGroup) and hasattr(native.FinishGroup, "run") and hasattr(native.FinishGroup, "close")
    assert hasattr(native.UpdateGroup, "stats_range")


def test_null_arguments_are_refused_without_a_gpu(lib):
    h = ctypes.c_void_p()
    assert lib.ddrl_finish_group_create(None, 1, ctypes.byref(h)) != 0
    assert b"null argument" in lib.ddrl_last_error()
    one = (ctypes.c_void_p * 1)(None)
    assert lib.ddrl_finish_group_create(one, 1, None) != 0
    assert b"null argument" in lib.ddrl_last_error()
    assert lib.ddrl_finish_group_create(one, 0, ctypes.byref(h)) != 0
    assert b"finish group: at least one member is needed" in lib.ddrl_last_error()
    assert lib.ddrl_finish_group_create(one, 1, ctypes.byref(h)) != 0
    assert b"finish group: member 0 is a null context" in lib.ddrl_last_error()
    assert lib.ddrl_finish_group_create(one, 65536, ctypes.byref(h)) != 0
    assert b"65535" in lib.ddrl_last_error()
    n = (ctypes.c_int64 * 1)()
    assert lib.ddrl_finish_group_run(None, n) != 0
    assert b"null finish group" in lib.ddrl_last_error()
    assert lib.ddrl_finish_group_rows(None, one, n) != 0
    assert b"null finish group" in lib.ddrl_last_error()
    assert lib.ddrl_update_group_stats_range(None, 0, 0, None) != 0
    assert b"null update group" in lib.ddrl_last_error()
    assert lib.ddrl_finish_group_destroy(None) == 0
