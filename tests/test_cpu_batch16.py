"""A context's capacity is 16 sequences (the 16 rows of the batched decode projections' MFMA tile): pgmi_create
accepts max_batch in [1, 16] and refuses everything else.  CPU only: pgmi_create builds the weight layout and
touches no device."""
import ctypes

import pytest


def _config(max_batch):
    from pgmi import _native as N
    from pgmi.engine import config_dict
    from pgmi.synthetic import paligemma_3b_config
    cd = config_dict(paligemma_3b_config())
    c = N.PgmiConfig()
    for k, _ in N.PgmiConfig._fields_:
        if k not in ("max_batch", "max_seq", "max_kv"):
            setattr(c, k, cd[k])
    c.max_batch, c.max_seq, c.max_kv = max_batch, 288, 1024
    return c


@pytest.mark.parametrize("max_batch", [9, 12, 16])
def test_create_accepts_up_to_16_rows(max_batch):
    from pgmi import _native as N
    lib = N.lib()
    c = _config(max_batch)
    h = ctypes.c_void_p()
    assert lib.pgmi_create(0, ctypes.byref(c), ctypes.byref(h)) == 0, lib.pgmi_last_error()
    # the KV cache of a full batch: layers x (K, V) x rows x tokens x 256 bf16
    assert lib.pgmi_kv_bytes(h, max_batch, 1024) == 18 * 2 * max_batch * 1024 * 256 * 2
    lib.pgmi_destroy(h)


@pytest.mark.parametrize("max_batch", [0, 17])
def test_create_refuses_outside_1_to_16(max_batch):
    from pgmi import _native as N
    lib = N.lib()
    c = _config(max_batch)
    h = ctypes.c_void_p()
    assert lib.pgmi_create(0, ctypes.byref(c), ctypes.byref(h)) == N.PGMI_E_ARG
    assert b"[1, 16]" in lib.pgmi_last_error()
    assert not h.value


def test_python_defaults_stay_at_8():
    import inspect

    from pgmi import binding
    from pgmi.engine import Engine
    assert binding.DEFAULT_MAX_BATCH == 8
    assert inspect.signature(Engine.__init__).parameters["max_batch"].default == 8
