"""The lossless 13-bit weight format of the batch 1-2 decode step, the parts that need no GPU: the numpy
statement of the format (pgmi/packed.py), the library's own host-side encode / decode -- the very functions the
pack kernel and the GEMV kernels are compiled from (csrc/pack13.h) -- against it, and the C entries' argument
checks on a context that owns no device memory."""
import ctypes

import numpy as np
import pytest

from pgmi import packed as P

K = 2048


def _random_bits(seed, n, e_hi=127, span=30, zeros=0.01):
    """bf16 patterns with exponent fields in [e_hi - span, e_hi] and a few exponent-0 elements."""
    rng = np.random.default_rng(seed)
    e = rng.integers(e_hi - span, e_hi + 1, n)
    e[0] = e_hi
    bits = (rng.integers(0, 2, n) << 15) | (e << 7) | rng.integers(0, 128, n)
    z = rng.random(n) < zeros
    z[0] = False
    bits[z] &= 0x807F   # exponent field 0: signed zeros and denormals
    return bits.astype(np.uint16)


def _edge_tensor(e_hi=130):
    """+0, -0, denormals of both signs, negative values, elements exactly at e_hi and e_hi - 30."""
    b = _random_bits(5, 2 * K, e_hi=e_hi, span=12, zeros=0.0)
    b[0] = e_hi << 7 | 0x55
    b[1], b[2] = 0x0000, 0x8000
    b[3], b[4], b[5] = 0x0001, 0x807F, 0x0040
    b[6] = (e_hi - 30) << 7
    b[7] = 0x8000 | (e_hi - 30) << 7 | 0x7F
    b[8] = 0x8000 | e_hi << 7 | 0x7F
    b[K - 1], b[K], b[2 * K - 1] = 0x8000, (e_hi - 30) << 7 | 1, 0x0001   # segment and row borders
    return b


@pytest.mark.parametrize("seed,e_hi,span", [(1, 127, 30), (2, 255, 30), (3, 31, 30), (4, 20, 19), (5, 124, 24)])
def test_pack_unpack_identity_np(seed, e_hi, span):
    b = _random_bits(seed, 5000, e_hi, span)
    assert P.e_hi_np(b) == e_hi and P.fits_np(b)
    sm, code = P.pack_np(b, e_hi)
    assert sm.dtype == np.uint8 and code.max() <= 31
    assert np.array_equal(P.unpack_np(sm, code, e_hi), b)


def test_edge_values_np():
    b = _edge_tensor()
    assert P.fits_np(b)
    sm, code = P.pack_np(b, 130)
    assert code[0] == 0 and code[6] == 30 and code[7] == 30 and (code[1:6] == 31).all()
    assert sm[2] == 0x80 and sm[4] == 0xFF and sm[8] == 0xFF
    assert np.array_equal(P.unpack_np(sm, code, 130), b)


def test_fit_rule():
    b = _edge_tensor(130)
    assert P.fits_np(b)
    bad = b.copy()
    bad[100] = (130 - 31) << 7          # one element one binade too low
    assert not P.fits_np(bad)
    with pytest.raises(ValueError):
        P.pack_np(bad, 130)
    only_zeros_small = np.full(K, 100 << 7 | 3, np.uint16)
    only_zeros_small[::7] = 0x8000      # the only small elements have exponent field 0
    only_zeros_small[1::7] = 0x0002
    assert P.fits_np(only_zeros_small)
    assert P.fits_np(np.zeros(K, np.uint16))   # e_hi = 0: every code is 31


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _c_roundtrip(lib, b, rows, k):
    e_hi, fits = ctypes.c_int(), ctypes.c_int()
    assert lib.pgmi_pack13_scan(_p(b), b.size, ctypes.byref(e_hi), ctypes.byref(fits)) == 0
    n = lib.pgmi_pack13_bytes(rows, k)
    assert n == P.image_bytes(rows, k) == rows * k * 13 // 8
    img = np.full(n + 64, 0xA5, np.uint8)   # guard bytes behind the image
    assert lib.pgmi_pack13_encode(_p(b), rows, k, e_hi.value, _p(img)) == 0
    assert (img[n:] == 0xA5).all()
    out = np.zeros_like(b)
    assert lib.pgmi_pack13_decode(_p(img), rows, k, e_hi.value, _p(out)) == 0
    return e_hi.value, bool(fits.value), img[:n], out


@pytest.mark.parametrize("case", ["random127", "random255", "low31", "tiny", "edges", "zeros"])
def test_library_image_roundtrip_matches_np(case):
    """The layout and the decode arithmetic the kernels run (pack13.h, compiled for the host): the image decodes
    to the input bit for bit, and scan agrees with the numpy rule."""
    from pgmi import _native as N
    lib = N.lib()
    rows, k = 3, 2 * K
    b = {"random127": lambda: _random_bits(11, rows * k, 127, 30),
         "random255": lambda: _random_bits(12, rows * k, 255, 30),
         "low31": lambda: _random_bits(13, rows * k, 31, 30),
         "tiny": lambda: _random_bits(14, rows * k, 9, 8),
         "edges": lambda: np.resize(_edge_tensor(), rows * k),
         "zeros": lambda: np.zeros(rows * k, np.uint16)}[case]()
    e_hi, fits, img, out = _c_roundtrip(lib, b, rows, k)
    assert e_hi == P.e_hi_np(b) and fits and P.fits_np(b)
    assert np.array_equal(out, b)
    # the sign/mantissa plane holds the numpy statement's bytes: lane l, chunk c, j -> weight 512 c + 8 l + j
    sm, _ = P.pack_np(b, e_hi)
    seg0 = img[:P.SEG_BYTES]
    for l in (0, 1, 37, 63):
        for c in range(4):
            want = sm[512 * c + 8 * l: 512 * c + 8 * l + 8]
            got = seg0[(c // 2) * 1024 + 16 * l + 8 * (c % 2):][:8]
            assert np.array_equal(got, want)


def test_library_scan_rejects_one_low_element():
    from pgmi import _native as N
    lib = N.lib()
    b = _edge_tensor(130)
    e_hi, fits = ctypes.c_int(), ctypes.c_int()
    assert lib.pgmi_pack13_scan(_p(b), b.size, ctypes.byref(e_hi), ctypes.byref(fits)) == 0
    assert (e_hi.value, fits.value) == (130, 1)
    b[777] = 0x8000 | (130 - 31) << 7
    assert lib.pgmi_pack13_scan(_p(b), b.size, ctypes.byref(e_hi), ctypes.byref(fits)) == 0
    assert (e_hi.value, fits.value) == (130, 0)


def _bare_ctx(N):
    """A context that owns no device memory (pgmi_create builds only the weight layout)."""
    from pgmi.engine import config_dict
    from oracle import weights as W
    cd = config_dict(W.small_config())
    c = N.PgmiConfig()
    for k, _ in N.PgmiConfig._fields_:
        if k not in ("max_batch", "max_seq", "max_kv"):
            setattr(c, k, cd[k])
    c.max_batch, c.max_seq, c.max_kv = 1, 64, 128
    h = ctypes.c_void_p()
    assert N.lib().pgmi_create(0, ctypes.byref(c), ctypes.byref(h)) == 0
    return h


def test_c_entries_refuse_bad_arguments_without_a_device():
    from pgmi import _native as N
    lib = N.lib()
    for name in ("pgmi_set_decode_packed", "pgmi_decode_packed_info", "pgmi_decode_packed_tensor",
                 "pgmi_pack13_scan", "pgmi_pack13_bytes", "pgmi_pack13_encode", "pgmi_pack13_decode"):
        assert name in N.SIGNATURES and hasattr(lib, name)
    info = (ctypes.c_int64 * 9)()
    p = 4096   # never dereferenced
    assert lib.pgmi_set_decode_packed(None, 1) == N.PGMI_E_ARG
    assert lib.pgmi_decode_packed_info(None, info, 9) == N.PGMI_E_ARG
    assert lib.pgmi_decode_packed_tensor(None, 1, 0) == N.PGMI_E_ARG
    assert b"null" in lib.pgmi_last_error()
    e, f = ctypes.c_int(), ctypes.c_int()
    assert lib.pgmi_pack13_scan(None, 8, ctypes.byref(e), ctypes.byref(f)) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_scan(p, 0, ctypes.byref(e), ctypes.byref(f)) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_scan(p, 8, None, ctypes.byref(f)) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_bytes(1, 1000) == -1 and lib.pgmi_pack13_bytes(0, K) == -1
    assert lib.pgmi_pack13_bytes(1, 0) == -1 and lib.pgmi_pack13_bytes(2, K) == 2 * 3328
    assert lib.pgmi_pack13_encode(None, 1, K, 127, p) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_encode(p, 1, K, 127, None) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_encode(p, 1, K + 8, 127, p) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_encode(p, 1, K, 256, p) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_decode(None, 1, K, 127, p) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_decode(p, 0, K, 127, p) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_decode(p, 1, K, -1, p) == N.PGMI_E_ARG
    h = _bare_ctx(N)
    try:
        assert lib.pgmi_decode_packed_info(h, None, 9) == N.PGMI_E_ARG
        assert lib.pgmi_decode_packed_info(h, info, 8) == N.PGMI_E_ARG
        assert lib.pgmi_set_decode_packed(h, 8) == N.PGMI_E_ARG
        assert lib.pgmi_decode_packed_tensor(h, 3, 0) == N.PGMI_E_ARG
        assert lib.pgmi_decode_packed_tensor(h, 1, 99) == N.PGMI_E_ARG
        assert lib.pgmi_decode_packed_tensor(h, 2, -1) == N.PGMI_E_ARG
        # a context that never decoded: the default mask, nothing packed yet, every candidate raw
        assert lib.pgmi_decode_packed_info(h, info, 9) == 0
        assert info[0] == P.ALL_KINDS and info[8] == P.KINDS["lm_head"] and info[1] == 0 and info[5] == 0 and info[6] == 0 and info[7] == 0
        assert lib.pgmi_decode_packed_tensor(h, 4, 0) == 0
        # a mask holds at B = 1 and B = 2 alike; the default is the kinds that measured faster at each batch
        for on, want, want2 in ((0, 0, 0), (5, 5, 5), (-1, P.ALL_KINDS, P.KINDS["lm_head"])):
            assert lib.pgmi_set_decode_packed(h, on) == 0
            assert lib.pgmi_decode_packed_info(h, info, 9) == 0 and (info[0], info[8]) == (want, want2)
    finally:
        lib.pgmi_destroy(h)
