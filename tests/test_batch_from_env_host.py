"""What of mmw_batch_create_from_env can be checked without a device: the header declares it and the built library exports it, and
the Python layer refuses a bad `handover` and a wrong-length `Zs` before anything reaches the library."""
import ctypes
import os
import re

import pytest

from sig_sdp_mmw_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_declares_the_entry_and_the_library_exports_it():
    with open(os.path.join(ROOT, "include", "mmw_hip.h")) as f:
        header = f.read()
    decl = re.search(r"int\s+mmw_batch_create_from_env\s*\(([^;]*)\)\s*;", header)
    assert decl, "mmw_batch_create_from_env is not declared in include/mmw_hip.h"
    args = " ".join(decl.group(1).split())
    assert args == "mmw_batch** out, mmw_batch_env* env, const int32_t* Z, int32_t rank_radio, double eta, const int32_t* nit"
    assert "mmw_batch_create_from_env" in _lib.EXPORTS
    assert getattr(_lib.lib(), "mmw_batch_create_from_env") is not None
    for name in ("MMW_F_PATTERN = %d" % _lib.BATCH_F_PATTERN, "MMW_F_BUILD_INFO = %d" % _lib.BATCH_F_BUILD_INFO, "MMW_I_PATTERN = %d" % _lib.I_PATTERN):
        assert name in header, name


def test_an_unknown_handover_is_refused_before_anything_runs():
    class Untouchable:
        """A drop whose every attribute is an error: the keyword is checked before the drops are looked at."""

        def __getattr__(self, name):
            raise AssertionError("online_resolve_many looked at a drop (%s) before it checked `handover`" % name)

    with pytest.raises(ValueError, match="handover must be"):
        batch.online_resolve_many([Untouchable()], handover="both")


def test_from_env_refuses_a_wrong_length_before_calling_the_library(monkeypatch):
    class Env:
        B = 3
        _h = ctypes.c_void_p()

    def no_library():
        raise AssertionError("BatchSolver.from_env called the library")

    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(_lib.MMWError, match="2 slot counts for the environment's 3 instances"):
        _lib.BatchSolver.from_env(Env(), [2, 2], 5, 0.04)
