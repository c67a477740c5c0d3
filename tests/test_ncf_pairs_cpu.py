"""The pair-scoring entry point (rg_ncf_score_pairs) without a GPU: the header declares it and its
tile constant, the ctypes table binds it with the documented argument types, the built library
exports it, and NCFEngine has both the kernel path (scores) and the torch path (scores_torch)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, TILE = "rg_ncf_score_pairs", "RG_NCF_SCORE_PAIR_TILE"


def header():
    return open(os.path.join(ROOT, "include", "rg_hip.h")).read()


def test_header_declares_the_function_and_tile_constant():
    txt = header()
    assert re.search(r"^\s*int\s+" + NAME + r"\s*\(", txt, flags=re.M)
    m = re.search(r"#define\s+" + TILE + r"\s+(\d+)", txt)
    assert m and int(m.group(1)) > 0 and int(m.group(1)) % 16 == 0


def test_binding_has_the_signature():
    from recommendation_gans_amd import _lib
    sig = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    assert NAME in sig
    res, args = sig[NAME]
    # (void *stream, const rg_ncf_model_t *model, const int64_t *users_dev, const int64_t *items_dev,
    #  int64_t n, float *out_dev)
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.POINTER(_lib.NCFModel), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                    ctypes.c_void_p]


def test_tile_constant_matches_the_header():
    from recommendation_gans_amd import _lib
    m = re.search(r"#define\s+" + TILE + r"\s+(\d+)", header())
    assert m and int(m.group(1)) == getattr(_lib, TILE)


def test_library_exports_the_symbol():
    from recommendation_gans_amd import _lib, build
    assert hasattr(ctypes.CDLL(build.build()), NAME)
    assert hasattr(_lib.load(), NAME)


def test_engine_has_both_paths():
    from recommendation_gans_amd.ncf_engine import NCFEngine
    assert callable(getattr(NCFEngine, "scores", None)) and callable(getattr(NCFEngine, "scores_torch", None))
    assert NCFEngine.scores is not NCFEngine.scores_torch
