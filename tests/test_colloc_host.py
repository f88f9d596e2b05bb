"""CPU-only checks of the element-wise collocation operators' host side: the
C ABI exports and the -kle_op_type option / opType keyword parsing.  Nothing
here touches the device."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


def test_colloc_symbols_are_exported_and_bound(pa):
    lib = C.CDLL(pa._lib.LIBPATH)
    bound = set(pa._lib.exported_symbols())
    for name in ("kle_mat_create_operator_element", "kle_element_ops"):
        assert hasattr(lib, name), name
        assert name in bound, name


def test_null_arguments_are_refused_before_the_device(pa):
    lib = C.CDLL(pa._lib.LIBPATH)
    lib.kle_mat_create_operator_element.restype = C.c_int
    out = C.c_void_p()
    rc = lib.kle_mat_create_operator_element(None, None, 0, C.byref(out))
    assert rc != 0 and not out.value


def test_op_type_option_and_keyword(pa):
    from pynama_amd.matrices import kle_op_type
    from pynama_amd.petsc import Options
    opts = Options()
    assert kle_op_type() == "assembled"
    assert kle_op_type("element") == "element" and kle_op_type("assembled") == "assembled"
    opts.setValue("kle_op_type", "element")
    try:
        assert kle_op_type() == "element"
        # the keyword wins over the option
        assert kle_op_type("assembled") == "assembled"
        # -kle_mat_type is another option
        from pynama_amd.matrices import kle_mat_type
        assert kle_mat_type() == "assembled"
    finally:
        opts.delValue("kle_op_type")
    assert kle_op_type() == "assembled"
    for bad in ("matrixfree", "", "Element"):
        opts.setValue("kle_op_type", bad)
        try:
            with pytest.raises(pa.Error) as ei:
                kle_op_type()
            assert ei.value.ierr == 62
        finally:
            opts.delValue("kle_op_type")
    with pytest.raises(pa.Error) as ei:
        kle_op_type("dense")
    assert ei.value.ierr == 62


def test_bad_option_stops_a_build_before_any_work(pa):
    """MatFS.build and Operators.build read the option before they touch the
    mesh or the device: a bad value raises 62 with nothing built."""
    from pynama_amd.matrices import MatFS, Operators
    from pynama_amd.petsc import Options

    class Dom:
        def getBoundaryType(self):
            return "FS"

        def getMesh(self):
            raise AssertionError("the mesh must not be reached")

        getDimensions = getMesh

    mat = MatFS()
    mat.setDomain(Dom())
    opts = Options()
    opts.setValue("kle_op_type", "sumfactorised")
    try:
        with pytest.raises(pa.Error) as ei:
            mat.build()
        assert ei.value.ierr == 62
        with pytest.raises(pa.Error) as ei:
            Operators().build(None)
        assert ei.value.ierr == 62
    finally:
        opts.delValue("kle_op_type")
    with pytest.raises(pa.Error) as ei:
        mat.build(opType="dense")
    assert ei.value.ierr == 62
    assert mat.K is None and mat.operator is None


def test_unknown_operator_name(pa):
    with pytest.raises(pa.Error) as ei:
        pa.petsc.Mat.createOperatorElement(None, "Div")
    assert ei.value.ierr == 62
