"""The fragment-major 13-bit image of the batched (3..16 rows) decode step, the parts that need no GPU: the numpy
statement of the gather and the byte layout (pgmi/packed.py) against the library's host-side encode / decode -- the
functions the pack kernel and the MFMA GEMVs are compiled from (csrc/pack13.h) -- byte for byte, and the new C
entries' argument checks on a context that owns no device memory."""
import ctypes

import numpy as np
import pytest

from pgmi import packed as P

K = 2048


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _random_bits(seed, shape, e_hi=127, span=30, zeros=0.01):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    e = rng.integers(e_hi - span, e_hi + 1, n)
    e[0] = e_hi
    bits = (rng.integers(0, 2, n) << 15) | (e << 7) | rng.integers(0, 128, n)
    z = rng.random(n) < zeros
    z[0] = False
    bits[z] &= 0x807F   # exponent field 0: signed zeros and denormals
    return bits.astype(np.uint16).reshape(shape)


def _c_image(lib, w, e_hi):
    rows, k = w.shape
    n = lib.pgmi_pack13_bytes_mf(rows, k)
    assert n == P.image_bytes_mf(rows, k) == P.mf_groups(rows) * 16 * k * 13 // 8
    img = np.full(n + 64, 0xA5, np.uint8)   # guard bytes behind the image
    assert lib.pgmi_pack13_encode_mf(_p(w), rows, k, e_hi, _p(img)) == 0
    assert (img[n:] == 0xA5).all()
    out = np.full((P.mf_groups(rows) * 16, k), 0x5A5A, np.uint16)   # the pad rows are written too
    assert lib.pgmi_pack13_decode_mf(_p(img), rows, k, e_hi, _p(out)) == 0
    return img[:n], out


def _check(lib, w, e_hi):
    rows, k = w.shape
    img, out = _c_image(lib, w, e_hi)
    # every byte, at every (segment, piece, lane) offset, is the numpy statement's
    want = P.encode_mf_np(w, e_hi)
    assert want.shape == img.shape and np.array_equal(img, want)
    assert np.array_equal(out[:rows], w)
    assert not out[rows:].any()   # pad rows decode to +0
    return img


@pytest.mark.parametrize("rows,k", [(16, K), (40, K), (32, 16384), (64, K)])
def test_library_image_is_the_numpy_statement_byte_for_byte(rows, k):
    """16 x 2048, 40 x 2048 (a partial last group), 32 x 16384 (the down shape's K), and the gate|up pair form of
    2 x 32 rows (one 64-row matrix: the up rows' groups after the gate rows')."""
    from pgmi import _native as N
    lib = N.lib()
    w = _random_bits(rows + k, (rows, k), 127, 30)
    e_hi, fits = ctypes.c_int(), ctypes.c_int()
    assert lib.pgmi_pack13_scan(_p(w), w.size, ctypes.byref(e_hi), ctypes.byref(fits)) == 0
    assert e_hi.value == P.e_hi_np(w) and fits.value == 1
    img = _check(lib, w, e_hi.value)
    if rows == 64:
        # the pair form: row set j (gate 0, up 1) of I = 32 rows, group gr, k block kb is segment
        # (j * n_groups + gr) * (K / 128) + kb, and holds that set's rows 16 gr .. + 15
        I, ng = 32, 2
        sm, _ = P.pack_np(w, e_hi.value)
        for j, gr, kb, l, c in ((0, 0, 0, 0, 0), (0, 1, 15, 63, 3), (1, 0, 0, 17, 1), (1, 1, 7, 42, 2)):
            seg = img[((j * ng + gr) * (k // 128) + kb) * P.SEG_BYTES:][:P.SEG_BYTES]
            row, k0 = j * I + 16 * gr + (l & 15), 128 * kb + 32 * c + 8 * (l >> 4)
            got = seg[(c // 2) * 1024 + 16 * l + 8 * (c % 2):][:8]
            assert np.array_equal(got, sm[row, k0:k0 + 8])


@pytest.mark.parametrize("e_hi", [130, 255, 31])
def test_crafted_values_at_the_corners(e_hi):
    """+-0, denormals, e_hi and e_hi - 30 at the first and last lane, chunk, k block and row of a group, and on both
    sides of a group boundary; the last group is partial (40 rows)."""
    from pgmi import _native as N
    lib = N.lib()
    rows = 40
    w = _random_bits(9, (rows, K), e_hi, 12, zeros=0.0)
    vals = [0x0000, 0x8000, 0x0001, 0x807F, 0x0040, e_hi << 7 | 0x55, 0x8000 | e_hi << 7 | 0x7F,
            (e_hi - 30) << 7, 0x8000 | (e_hi - 30) << 7 | 0x7F]
    # lane l = (n, g), chunk c, j, k block kb -> row 16 gr + n, k = 128 kb + 32 c + 8 g + j
    corners = [(r, 128 * kb + 32 * c + 8 * g + j)
               for r in (0, 15, 16, 31, 32, 39)             # first / last row of a group, both sides of two borders
               for kb in (0, K // 128 - 1) for c in (0, 3) for g in (0, 3) for j in (0, 7)]
    for i, (r, k) in enumerate(corners):
        w[r, k] = vals[i % len(vals)]
    w[0, 0] = e_hi << 7     # the tensor's largest exponent stays e_hi
    assert P.e_hi_np(w) == e_hi and P.fits_np(w)
    _check(lib, w, e_hi)
    zeros = np.zeros((17, K), np.uint16)
    _check(lib, zeros, 0)   # e_hi = 0: every code is 31


def test_index_map_is_the_bf16_fragment_major_image():
    """k_mf_swizzle's comment: 16-B chunk (row group gr, 32-k block kb32, lane l) at element offset
    ((gr * K / 32 + kb32) * 64 + l) * 8 holds row 16 gr + (l & 15), k = 32 kb32 + 8 (l >> 4) .. + 8.  The packed
    image's (group, 128-k block, lane, chunk c) is that image's (group, 32-k block 4 kb + c, lane): the same
    (row, k) per (group, k block, lane, j)."""
    rows, k = 48, 4096
    r, kk = P.frag_index_np(rows, k)
    assert r.shape == kk.shape == (3, k // 128, 64, 4, 8)
    gr, kb, l, c, j = np.meshgrid(np.arange(3), np.arange(k // 128), np.arange(64), np.arange(4), np.arange(8),
                                  indexing="ij")
    kb32 = 4 * kb + c
    assert np.array_equal(r, 16 * gr + (l & 15))
    assert np.array_equal(kk, 32 * kb32 + 8 * (l >> 4) + j)
    # and through the offsets: gathering a row-major matrix by (r, kk) is reading the swizzled image in order
    w = np.arange(rows * k, dtype=np.int64).reshape(rows, k)
    off = ((gr * (k // 32) + kb32) * 64 + l) * 8 + j
    swz = np.empty(rows * k, np.int64)
    swz[off.reshape(-1)] = w[r, kk].reshape(-1)
    lanes = np.arange(64)
    for g_, b_ in ((0, 0), (2, k // 32 - 1), (1, 17)):
        chunk = swz[(g_ * (k // 32) + b_) * 512:][:512].reshape(64, 8)
        want = w[(16 * g_ + (lanes & 15))[:, None], (32 * b_ + 8 * (lanes >> 4))[:, None] + np.arange(8)[None, :]]
        assert np.array_equal(chunk, want)
    # every weight exactly once
    assert np.array_equal(np.sort((r * k + kk).reshape(-1)), np.arange(rows * k))


def _read_back(img):
    """(sign|mantissa byte, stored 5-bit value u = 31 - code) of every weight of an image's segments, each
    [segments][64 lanes][4 chunks][8]: seg_image_np's byte layout (pgmi/packed.py) read the other way."""
    seg = np.ascontiguousarray(img).reshape(-1, P.SEG_BYTES)
    n = seg.shape[0]
    sm = np.concatenate([seg[:, 0:1024].reshape(n, 64, 2, 8), seg[:, 1024:2048].reshape(n, 64, 2, 8)], axis=2)
    j = np.arange(8)
    nib = np.ascontiguousarray(seg[:, 2048:3072]).view("<u4").reshape(n, 64, 4)
    low = (nib[..., None] >> (16 * (j & 1) + 4 * (j >> 1)).astype(np.uint32)) & 15
    hi = np.ascontiguousarray(seg[:, 3072:3328]).view("<u4").reshape(n, 64)
    c = np.arange(4)[:, None]
    top = (hi[..., None, None] >> (16 * (j & 1)[None, :] + 4 * c + (j >> 1)[None, :]).astype(np.uint32)) & 1
    return sm, (low | (top << 4)).astype(np.uint8)


def test_both_forms_hold_the_same_record_of_every_weight():
    """Same record, two gathers: one fitting 40 x 4096 matrix (a partial last group; two row-major segments per row,
    32 k blocks) through both encoders.  Every weight's 13 bits -- its sign|mantissa byte and its stored 5-bit value
    (u = 31 - code: what the planes hold) -- read back with numpy at the offsets of each form, agree between the two
    images and with pack_np; the fragment image's pad rows hold byte 0 and stored value 0 (a zero: code 31)."""
    from pgmi import _native as N
    lib = N.lib()
    rows, k = 40, 4096
    w = _random_bits(77, (rows, k), 127, 30)
    e_hi = P.e_hi_np(w)
    assert P.fits_np(w)
    n_r, n_f = lib.pgmi_pack13_bytes(rows, k), lib.pgmi_pack13_bytes_mf(rows, k)
    assert n_r == P.image_bytes(rows, k) and n_f == P.image_bytes_mf(rows, k)
    img_r, img_f = np.zeros(n_r, np.uint8), np.zeros(n_f, np.uint8)
    assert lib.pgmi_pack13_encode(_p(w), rows, k, e_hi, _p(img_r)) == 0
    assert lib.pgmi_pack13_encode_mf(_p(w), rows, k, e_hi, _p(img_f)) == 0
    # row-major: segment row * (K / 2048) + s, lane l, chunk c, j holds k = 2048 s + 512 c + 8 l + j of that row
    row, s, l, c, j = np.meshgrid(np.arange(rows), np.arange(k // P.SEG_WEIGHTS), np.arange(64), np.arange(4),
                                  np.arange(8), indexing="ij")
    kk = P.SEG_WEIGHTS * s + 512 * c + 8 * l + j
    by_form = []
    for img, (r_i, k_i) in ((img_r, (row, kk)), (img_f, P.frag_index_np(rows, k))):
        sm, u = _read_back(img)
        sm, u = sm.reshape(r_i.shape), u.reshape(r_i.shape)
        real = r_i < rows
        assert real.sum() == rows * k   # every weight exactly once (the index arrays are permutations of it)
        sm_w, u_w = np.full((rows, k), 0xEE, np.uint8), np.full((rows, k), 0xEE, np.uint8)
        sm_w[r_i[real], k_i[real]] = sm[real]
        u_w[r_i[real], k_i[real]] = u[real]
        by_form.append((sm_w, u_w))
        assert not sm[~real].any() and not u[~real].any()   # pad rows (the fragment form's rows 40..47)
    assert (~(P.frag_index_np(rows, k)[0] < rows)).sum() == 8 * k
    (sm_r, u_r), (sm_f, u_f) = by_form
    assert np.array_equal(sm_r, sm_f) and np.array_equal(u_r, u_f)
    want_sm, want_code = P.pack_np(w, e_hi)
    assert np.array_equal(sm_r, want_sm) and np.array_equal(u_r, 31 - want_code)


def test_refusals_and_setters_without_a_device():
    from pgmi import _native as N
    from test_cpu_packed import _bare_ctx
    lib = N.lib()
    for name in ("pgmi_set_decode_packed_batched", "pgmi_decode_packed_batched_info",
                 "pgmi_decode_packed_batched_tensor", "pgmi_pack13_bytes_mf", "pgmi_pack13_encode_mf",
                 "pgmi_pack13_decode_mf"):
        assert name in N.SIGNATURES and hasattr(lib, name)
    p = 4096   # never dereferenced
    assert lib.pgmi_pack13_bytes_mf(1, 1000) == -1 and lib.pgmi_pack13_bytes_mf(0, K) == -1
    assert lib.pgmi_pack13_bytes_mf(16, K + 128) == -1 and lib.pgmi_pack13_bytes_mf(-3, K) == -1
    assert lib.pgmi_pack13_bytes_mf(1, K) == lib.pgmi_pack13_bytes_mf(16, K) == 16 * 3328
    assert lib.pgmi_pack13_bytes_mf(17, 2 * K) == 2 * 32 * 3328
    assert lib.pgmi_pack13_encode_mf(None, 16, K, 127, p) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_encode_mf(p, 16, K, 127, None) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_encode_mf(p, 16, K + 128, 127, p) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_encode_mf(p, 0, K, 127, p) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_encode_mf(p, 16, K, 256, p) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_encode_mf(p, 16, K, -1, p) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_decode_mf(None, 16, K, 127, p) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_decode_mf(p, 0, K, 127, p) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_decode_mf(p, 16, 1000, 127, p) == N.PGMI_E_ARG
    assert lib.pgmi_pack13_decode_mf(p, 16, K, 256, p) == N.PGMI_E_ARG
    info = (ctypes.c_int64 * 6)()
    old = (ctypes.c_int64 * 9)()
    assert lib.pgmi_set_decode_packed_batched(None, 1) == N.PGMI_E_ARG
    assert lib.pgmi_decode_packed_batched_info(None, info, 6) == N.PGMI_E_ARG
    assert lib.pgmi_decode_packed_batched_tensor(None, 1, 0) == N.PGMI_E_ARG
    h = _bare_ctx(N)
    try:
        assert lib.pgmi_decode_packed_batched_info(h, None, 6) == N.PGMI_E_ARG
        assert lib.pgmi_decode_packed_batched_info(h, info, 5) == N.PGMI_E_ARG
        # the default: off, nothing scanned or packed, every candidate raw
        assert lib.pgmi_decode_packed_batched_info(h, info, 6) == 0
        assert list(info)[:3] == [0, 0, 0] and info[4] == 0 and info[5] == 0 and info[3] >= 1
        for bad in (8, 9, -1, -7):
            assert lib.pgmi_set_decode_packed_batched(h, bad) == N.PGMI_E_ARG
            assert b"decode_packed_batched" in lib.pgmi_last_error()
        assert lib.pgmi_decode_packed_batched_tensor(h, 3, 0) == N.PGMI_E_ARG
        assert lib.pgmi_decode_packed_batched_tensor(h, 1, 99) == N.PGMI_E_ARG
        assert lib.pgmi_decode_packed_batched_tensor(h, 2, -1) == N.PGMI_E_ARG
        assert lib.pgmi_decode_packed_batched_tensor(h, 4, 0) == 0
        for mask in (5, 7, 0):
            assert lib.pgmi_set_decode_packed_batched(h, mask) == 0
            assert lib.pgmi_decode_packed_batched_info(h, info, 6) == 0 and info[0] == mask and info[2] == 0
            # the B <= 2 calls keep their meaning and values: n = 9, the default masks, nothing packed
            assert lib.pgmi_decode_packed_info(h, old, 9) == 0
            assert old[0] == P.ALL_KINDS and old[8] == P.KINDS["lm_head"]
            assert old[1] == 0 and old[5] == 0 and old[6] == 0 and old[7] == 0
        assert lib.pgmi_decode_packed_info(h, old, 8) == N.PGMI_E_ARG
        assert lib.pgmi_set_decode_packed(h, 8) == N.PGMI_E_ARG
        # and the other way round: the B <= 2 switch leaves the batched mask alone
        assert lib.pgmi_set_decode_packed_batched(h, 3) == 0 and lib.pgmi_set_decode_packed(h, 0) == 0
        assert lib.pgmi_decode_packed_batched_info(h, info, 6) == 0 and info[0] == 3
        assert lib.pgmi_decode_packed_info(h, old, 9) == 0 and (old[0], old[8]) == (0, 0)
    finally:
        lib.pgmi_destroy(h)
