"""sparsepoly_amd.kernels on the host: the reference's names and signatures (sparsepoly/kernels.py
:14-153), safe_power, the checks that run before any device work, and loud failure without a
GPU.  No device compute here."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sp

# the reference's signatures, plus the keyword-only device of the device functions
EXPECTED = {
    "safe_power": [("X", inspect.Parameter.empty), ("degree", 2)],
    "homogeneous_kernel": [("X", inspect.Parameter.empty), ("P", inspect.Parameter.empty),
                           ("degree", 2)],
    "anova_kernel": [("X", inspect.Parameter.empty), ("P", inspect.Parameter.empty),
                     ("degree", 2)],
    "all_subsets_kernel": [("X", inspect.Parameter.empty), ("P", inspect.Parameter.empty)],
    "poly_predict": [("X", inspect.Parameter.empty), ("P", inspect.Parameter.empty),
                     ("lams", inspect.Parameter.empty), ("kernel", inspect.Parameter.empty),
                     ("degree", 2)],
}


def _has_gpu():
    import ctypes

    from sparsepoly_amd import _capi

    try:
        lib = _capi.load()
    except RuntimeError:
        return False
    h = ctypes.c_void_p()
    if lib.spfm_create(ctypes.byref(h), 0, 1) != 0:
        return False
    lib.spfm_destroy(h)
    return True


def test_module_exposes_reference_names_and_signatures():
    from sparsepoly_amd import kernels

    for name, params in EXPECTED.items():
        f = getattr(kernels, name)
        sig = inspect.signature(f)
        pos = [(p.name, p.default) for p in sig.parameters.values()
               if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]
        assert pos == params, name
        kwonly = [p for p in sig.parameters.values() if p.kind == inspect.Parameter.KEYWORD_ONLY]
        if name == "safe_power":
            assert kwonly == []
        else:
            assert [(p.name, p.default) for p in kwonly] == [("device", None)], name


def test_module_is_not_exported_from_package():
    import sparsepoly_amd

    assert "kernels" not in sparsepoly_amd.__all__
    for name in EXPECTED:
        assert name not in sparsepoly_amd.__all__


@pytest.mark.parametrize("fmt", ["dense", "csr", "csc"])
@pytest.mark.parametrize("degree", [1, 2, 3])
def test_safe_power_matches_numpy_and_scipy(fmt, degree):
    from sparsepoly_amd.kernels import safe_power

    rng = np.random.RandomState(0)
    Xd = rng.randn(7, 5) * (rng.rand(7, 5) < 0.5)
    X = Xd if fmt == "dense" else getattr(sp, fmt + "_matrix")(Xd)
    Y = safe_power(X, degree)
    if fmt == "dense":
        assert isinstance(Y, np.ndarray)
        np.testing.assert_array_equal(Y, Xd ** degree)
    else:
        assert sp.issparse(Y) and Y.format == fmt
        np.testing.assert_array_equal(Y.toarray(), X.power(degree).toarray())
        np.testing.assert_array_equal(Y.toarray(), Xd ** degree)
    np.testing.assert_array_equal(np.asarray(X if fmt == "dense" else X.toarray()), Xd)


def test_poly_predict_unknown_kernel_message():
    from sparsepoly_amd.kernels import poly_predict

    with pytest.raises(ValueError) as ei:
        poly_predict(np.ones((3, 4)), np.ones((2, 4)), np.ones(2), "foo")
    assert str(ei.value) == ("Unsuppported kernel: foo. Use one of "
                             "{'anova'|'poly'|'all-subsets'}")


@pytest.mark.parametrize("fn", ["homogeneous_kernel", "anova_kernel", "all_subsets_kernel",
                                "poly_predict"])
def test_shape_errors_before_device(fn):
    from sparsepoly_amd import kernels

    f = getattr(kernels, fn)
    extra = (np.ones(2), "anova") if fn == "poly_predict" else ()
    with pytest.raises(ValueError):  # feature-count mismatch
        f(np.ones((3, 4)), np.ones((2, 5)), *extra)
    with pytest.raises(ValueError):
        f(sp.csr_matrix(np.ones((3, 4))), np.ones((2, 5)), *extra)
    with pytest.raises(ValueError):  # 1-D input
        f(np.ones(4), np.ones((2, 4)), *extra)
    with pytest.raises(ValueError):
        f(np.ones((3, 4)), np.ones(4), *extra)


def test_degree_errors_before_device():
    from sparsepoly_amd.kernels import anova_kernel, homogeneous_kernel

    X, P = np.ones((3, 4)), np.ones((2, 4))
    with pytest.raises(NotImplementedError):
        anova_kernel(X, P, 65)
    for bad in (-1, 2.5):
        with pytest.raises(NotImplementedError):
            homogeneous_kernel(X, P, bad)


def test_device_functions_raise_without_gpu():
    """No CPU fallback: without a device (on a GPU machine: a device that does not exist) every
    device function raises SpfmError."""
    from sparsepoly_amd import kernels
    from sparsepoly_amd.engine import SpfmError

    X = sp.random(5, 4, density=0.5, format="csr", random_state=0)
    P = np.ones((2, 4))
    kw = {"device": 4096} if _has_gpu() else {}
    for call in (lambda: kernels.anova_kernel(X, P, 2, **kw),
                 lambda: kernels.homogeneous_kernel(X, P, 2, **kw),
                 lambda: kernels.all_subsets_kernel(X, P, **kw),
                 lambda: kernels.poly_predict(X, P, np.ones(2), "anova", 2, **kw)):
        with pytest.raises(SpfmError):
            call()
