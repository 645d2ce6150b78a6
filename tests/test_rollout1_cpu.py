"""CPU checks of the one-hidden-layer one-launch rollout's C ABI: the header declares the six
gs_rollout1_* entries, the built library exports them, the binding declares argument lists of the
header's lengths (and its siblings' types), and the ABI version did not move."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("gs_rollout1_supported", "gs_rollout1_env", "gs_rollout1_cartpole_shaped", "gs_rollout1_mountaincar",
               "gs_rollout1_bandit", "gs_rollout1_tabular")
SIBLINGS = {"gs_rollout1_env": "gs_rollout_env", "gs_rollout1_cartpole_shaped": "gs_rollout_cartpole_shaped",
            "gs_rollout1_mountaincar": "gs_rollout_mountaincar", "gs_rollout1_bandit": "gs_rollout_bandit"}


def _header():
    src = open(os.path.join(ROOT, "include", "gsamd.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _declared_args(src, name):
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_library_and_binding_agree_on_the_new_entries():
    from gsamd import _lib
    src = _header()
    declared = set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", src))
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTED and hasattr(_lib.lib, name), name
        args = _declared_args(src, name)
        assert len(getattr(_lib.lib, name).argtypes) == len(args), (name, len(args))
    assert declared == set(_lib.EXPORTED)
    # the four entries that share a sibling's argument list: the same C types in the same order
    strip = lambda a: re.sub(r"\s*\w+$", "", a)        # noqa: E731  (drop the parameter's name)
    for new, old in SIBLINGS.items():
        assert [strip(a) for a in _declared_args(src, new)] == [strip(a) for a in _declared_args(src, old)], new
        assert list(getattr(_lib.lib, new).argtypes) == list(getattr(_lib.lib, old).argtypes), new
    tab = _declared_args(src, "gs_rollout1_tabular")
    assert len(tab) == 30 and tab[11].startswith("gs_tabular_spec") and tab[-1] == "void *stream"
    assert getattr(_lib.lib, "gs_rollout1_tabular").argtypes[11] is _lib.TabularSpec


def test_abi_version_is_unchanged():
    from gsamd import _lib
    assert _lib.lib.gs_abi_version() == _lib.GS_ABI_VERSION == 7
    assert re.search(r"#define GS_ABI_VERSION 7\b", _header())


def test_supported_query_needs_no_device():
    """gs_rollout1_supported is a host computation: 1 for the presets' shapes, an error (and 0) for
    two hidden layers or a shape outside the one-hidden-layer envelope."""
    import ctypes

    import pytest
    from gsamd._lib import MlpDims, check, lib
    for dims in ((1, 64, 0, 4), (1, 64, 0, 6), (64, 64, 0, 32)):
        v = ctypes.c_int(7)
        check(lib.gs_rollout1_supported(MlpDims(*dims), ctypes.byref(v)), "gs_rollout1_supported")
        assert v.value == 1, dims
    for dims, msg in (((4, 256, 256, 2), "one hidden layer"), ((4, 40, 0, 4), "multiple of 16"),
                      ((64, 1024, 0, 4), r"\d+ bytes")):
        v = ctypes.c_int(7)
        with pytest.raises(ValueError, match=msg):
            check(lib.gs_rollout1_supported(MlpDims(*dims), ctypes.byref(v)), "gs_rollout1_supported")
        assert v.value == 0, dims
