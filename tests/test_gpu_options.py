"""GPU suite: the real entry points over the option table and the info names
(csrc/snapmi_options.hpp; tests/test_options_cpu.py holds the table itself
against written-out defaults and bounds).  A fresh context, no codec kernel:
every option takes its own default through the entry point it belongs to and
refuses a value outside its range with the text the setters always gave,
every info name answers its "no call yet" value, unknown names are
SNAPMI_E_ARGUMENT, and the shipped library refuses the test build's
cross-checks."""
import ctypes as C

import pytest
import torch

from conftest import product_context
from test_options_cpu import (INFO, INFO_TEST_BUILD, PRODUCT, SETS, TEST,
                              TEST_BUILD_WIDER, options_table)

pytestmark = pytest.mark.gpu

OK, E_ARGUMENT = 0, 101


@pytest.fixture(scope="module")
def fresh(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rust_snappy_amd as R
    c = R.raw.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shipped(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = product_context()
    yield c
    c.close()


def setter(ctx, test_only):
    L = ctx._L
    return (L.snapmi_ctx_set_test_option if test_only
            else L.snapmi_ctx_set_option)


def last_error(ctx):
    return ctx._L.snapmi_last_error(ctx._h).decode()


def get_info(ctx, name):
    v = C.c_int64(-777)
    rc = ctx._L.snapmi_ctx_get_info(ctx._h, name.encode(), C.byref(v))
    return rc, v.value


def own_default(name, default):
    """What "its own default" is for a name: the field's; the two names
    without a field: the device's own answer / the one value there is."""
    return {"lds_order_ok": 1, "lane_tables_renew": 1}.get(name, default)


def refused_value(name):
    """One value outside what the option takes in the test build, from the
    written-out bounds of test_options_cpu (scratch_fill: -2, which fills
    nothing)."""
    if name in SETS:
        return SETS[name][3][0]
    if name in TEST_BUILD_WIDER:
        return TEST_BUILD_WIDER[name][0] - 1
    return dict(PRODUCT, **TEST)[name][1] - 1


# (what a context holds before any call; no option below changes it)
def test_every_info_name_answers_its_no_call_yet_value(fresh):
    T = options_table()
    assert set(T.info) == set(INFO) | set(INFO_TEST_BUILD)
    for name in T.info_names:
        rc, v = get_info(fresh, name)
        assert rc == OK, (name, last_error(fresh))
        if name == "frame_nowait_front":
            assert v == -1
        elif name in ("scratch_bytes", "token_pool_pct_now"):
            assert v >= 0, name
        else:
            assert v == 0, (name, v)


def test_every_option_takes_its_default_and_refuses_a_value_outside(fresh):
    T = options_table()
    assert set(T.options) == set(PRODUCT) | set(TEST) | set(SETS)
    for name, (test_only, default) in T.options.items():
        f, text = setter(fresh, test_only), \
            ("unknown test option " if test_only else "unknown option ") + name
        assert f(fresh._h, name.encode(), own_default(name, default)) == OK, \
            (name, last_error(fresh))
        assert f(fresh._h, name.encode(), refused_value(name)) == E_ARGUMENT, \
            name
        assert last_error(fresh) == text
        # the other entry point does not know the name
        g = setter(fresh, not test_only)
        assert g(fresh._h, name.encode(), own_default(name, default)) == \
            E_ARGUMENT, name
        assert name in last_error(fresh)


def test_unknown_names(fresh):
    for test_only in (False, True):
        assert setter(fresh, test_only)(fresh._h, b"no_such_name", 1) == \
            E_ARGUMENT
        assert last_error(fresh) == (
            "unknown test option " if test_only else "unknown option "
        ) + "no_such_name"
    assert get_info(fresh, "no_such_name") == (E_ARGUMENT, -777)
    assert last_error(fresh) == "unknown info: no_such_name"


def test_shipped_library_refuses_the_cross_checks(fresh, shipped):
    L = shipped._L
    assert not hasattr(L, "snapmi_ctx_set_test_option")
    for name, v in (("span_kernel", 0), ("compress_mode", 2),
                    ("decode_kernel", 2)):
        assert L.snapmi_ctx_set_option(shipped._h, name.encode(), v) == \
            E_ARGUMENT, name
        assert last_error(shipped) == "unknown option " + name
        # (the test build takes them)
        assert setter(fresh, False)(fresh._h, name.encode(), v) == OK, name
    T = options_table()
    for name, (test_only, default) in T.options.items():
        rc = L.snapmi_ctx_set_option(shipped._h, name.encode(),
                                     own_default(name, default))
        assert rc == (E_ARGUMENT if test_only else OK), name
    for name, test_only in T.info.items():
        rc, _ = get_info(shipped, name)
        assert rc == (E_ARGUMENT if test_only else OK), name
    # put the test build's context back to its defaults
    for name, v in (("span_kernel", 1), ("compress_mode", 1),
                    ("decode_kernel", 3)):
        assert setter(fresh, False)(fresh._h, name.encode(), v) == OK
