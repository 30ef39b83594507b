"""CPU-side checks of the drop-in boundary: the library loads and exports every
symbol include/topopt_amd.h declares (no compute without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "topopt_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(tp_[a-z0-9_]+)\s*\(", src)))


def test_header_and_binding_agree():
    from topopt_in_petsc_amd import lib
    assert sorted(lib.SYMBOLS) == _declared()


def test_library_exports_every_declared_symbol():
    from topopt_in_petsc_amd import lib
    so = lib.build()
    dll = ctypes.CDLL(so)
    for name in _declared():
        assert hasattr(dll, name), "libtopopt_amd.so lacks %s" % name
    assert lib.load_library() is not None


def test_default_options_match_reference_defaults():
    from topopt_in_petsc_amd import lib, SolverOptions
    o = lib.SolverOpts()
    lib.load_library().tp_solver_default_opts(ctypes.byref(o))
    # LinearElasticity.cc:22-23, :621-635
    assert (o.nlvls, o.nu, o.rtol, o.atol, o.dtol, o.max_it, o.nsmooth, o.ncoarse) == (4, 0.3, 1e-5, 1e-50, 1e5, 200, 4, 30)
    d = SolverOptions()
    assert (d.nlvls, d.nu, d.rtol, d.max_it, d.nsmooth, d.ncoarse, d.cheb_lo, d.cheb_hi) == \
        (o.nlvls, o.nu, o.rtol, o.max_it, o.nsmooth, o.ncoarse, o.cheb_lo, o.cheb_hi)


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import topopt_in_petsc_amd as tp
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tp.Grid(9, 5, 5, 0.25)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "topopt_in_petsc_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert "oracle" not in txt.replace("no CPU fallback", "").lower() or f == "__init__.py" and False, \
                    "%s mentions the oracle" % f


CSRC = os.path.join(ROOT, "topopt_in_petsc_amd", "csrc")


def test_only_switches_h_reads_the_environment():
    """every environment variable of the product library has its accessor in csrc/switches.h; no other file there reads one"""
    readers = sorted(f for f in os.listdir(CSRC) if "getenv" in open(os.path.join(CSRC, f)).read())
    assert readers == ["switches.h"], readers


def test_only_common_h_allocates_device_memory():
    """device memory has one owner type, DevBuf of csrc/common.h, and the two raw helpers behind tp_malloc / tp_free beside it; no
    other file there allocates or frees any"""
    users = sorted(f for f in os.listdir(CSRC)
                   if any(call in open(os.path.join(CSRC, f)).read() for call in ("hipMalloc(", "hipFree(")))
    assert users == ["common.h"], users


# The library switches that bench.py, tests/*.py and tools/*.py put into the environment of a process that loads the
# library, by the file that sets them.  An explicit list: TP_BENCH_*, TP_CHECK_OUT, TP_ERR_*, TP_LIB, TP_RANK, ... are not
# library switches.  A name added to one of these files belongs here as well; a name may leave this list only with the
# code that sets it.
SWITCHES_SET_BY_NAME = {
    "bench.py": ["TP_NO_TILE", "TP_NO_MACRO", "TP_FINE_V", "TP_NO_PDE_STENCIL"],
    "tests/test_gpu_fine_generations.py": ["TP_FINE_V", "TP_FINE_SHAPE", "TP_TILE_KZ", "TP_NO_MACRO", "TP_DIA_NODE", "TP_DIA_SPLIT",
                                           "TP_NO_DIA_SYM", "TP_LANCZOS_ON_MAIN", "TP_LANCZOS_TAILS", "TP_NO_REDUCE_TAIL"],
    "tests/test_gpu_configs.py": ["TP_SMOOTH_GRAPH", "TP_COARSE_RUN", "TP_NO_COARSE_RUN", "TP_NO_COARSE_XCD", "TP_NO_LANCZOS_XCD",
                                  "TP_DEBUG_SYNC"],
    "tests/test_gpu_parity.py": ["TP_TEST_FORCE_GIVEUP", "TP_NO_COARSE_DIRECT", "TP_NO_COARSE_XCD", "TP_NO_LANCZOS_XCD",
                                 "TP_CD_INVERT_COLUMNS", "TP_NO_FILTER_TILE", "TP_FILTER_ZMULTI", "TP_NO_REDUCE_TAIL"],
    "tests/test_multirank.py": ["TP_REPLICATE_FROM", "TP_TEST_FORCE_GIVEUP", "TP_FINE_V", "TP_FINE_SHAPE"],
    "tests/test_gpu_rowwise.py": ["TP_FINE_V", "TP_FINE_SHAPE", "TP_TILE_KZ", "TP_NO_TILE", "TP_NO_MACRO", "TP_NO_CORR_FUSE", "TP_DIA_SPLIT",
                                  "TP_DIA_NODE", "TP_NO_DIA_SYM", "TP_MACRO_KZ", "TP_FILTER_ZMULTI", "TP_NO_FILTER_TILE"],
    "tests/rowwise_worker.py": ["TP_MACRO_KZ"],
    "tests/test_gpu_cg_fusions.py": ["TP_NO_FUSE_FIRST", "TP_NO_CG_FUSE", "TP_NO_SPEC_HEAD", "TP_NO_FUSE_RZ", "TP_CG_NT"],
    "tests/test_gpu_pde_rowwise.py": ["TP_NO_PDE_STENCIL"],
    "tests/mp_gloo_worker.py": ["TP_OVERLAP", "TP_TEST_FORCE_GIVEUP", "TP_FINE_V", "TP_FINE_SHAPE"],
    "tools/fine_ab.py": ["TP_FINE_V", "TP_TILE_KZ"],
    "tools/r06_c3_hist_variants.py": ["TP_DIA_NODE", "TP_NO_DIA_SYM"],
    "tools/r06_filter_ab.py": ["TP_FILTER_ZMULTI"],
}


def test_every_switch_set_by_name_exists():
    """a switch that the benchmark, a test or a tool sets must exist in the library: dropped or renamed, it would be ignored silently"""
    header = open(os.path.join(CSRC, "switches.h")).read()
    for path, names in SWITCHES_SET_BY_NAME.items():
        txt = open(os.path.join(ROOT, path)).read()
        for name in names:
            assert re.search(r"\b%s\b" % name, txt), "%s no longer names %s: update SWITCHES_SET_BY_NAME" % (path, name)
            assert '"%s"' % name in header, "%s sets %s, which csrc/switches.h does not read" % (path, name)
