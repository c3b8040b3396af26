"""Dynamically quantised models (the registry's *Q entries; the reference's DEFAULT model is one,
/root/reference/src/embed/embedder.rs:12-13): csrc/gemm_q8.hip through the C ABI.

Two bars.  (1) Operator level — the same activations in, the same integers out: DynamicQuantizeLinear's bytes and
parameters and MatMulInteger's int32 results are compared EXACTLY with a numpy statement of the ONNX definitions, and
the f32 scale / bias / residual stage bit for bit.  (2) Model level — against oracle/bert_oracle.c's quantised forward:
an 8-bit rounding sits behind every Linear, so two f32-class evaluations of the same graph (different summation order in
LayerNorm, another erf) disagree on a handful of activation bytes per tensor — a few 1e-4 on an embedding component;
the bar is therefore statistical (cosine and max error), and the test shows the quantised forward is what was run by
comparing against the f32 graph of the same weights, which sits an order of magnitude further away."""
import ctypes as C

import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd._lib import f32p
from codesearch_amd.bert_params import (POOL_CLS, POOL_MEAN, BertConfig, quant_columns, quantize_linear_weights,
                                        synth_params, synth_token_batch)
from tests.q8_ln_ref import dynamic_quantize, quantize_matrix, split_round_trip

pytestmark = pytest.mark.gpu


def run_q8(lib, epi, A, W, sc, bias, resid=None, a_split=0):
    M, K = A.shape
    N = W.shape[0]
    C_ = np.empty((M, N), np.float32)
    xq = np.empty((M, K), np.uint8)
    xp = np.empty(2, np.float32)
    acc = np.empty((M, N), np.int32)
    _lib.check_diag(lib.cs_debug_gemm_q8(0, epi, a_split, A.ctypes.data_as(f32p), W.ctypes.data_as(f32p), sc.ctypes.data_as(f32p),
                                    bias.ctypes.data_as(f32p), None if resid is None else resid.ctypes.data_as(f32p),
                                    C_.ctypes.data_as(f32p), M, N, K, xq.ctypes.data_as(C.POINTER(C.c_uint8)),
                                    xp.ctypes.data_as(f32p), acc.ctypes.data_as(C.POINTER(C.c_int32))))
    return C_, xq, xp, acc


# (from 4,096 rows on a K = 384 layer runs on the row-block kernel, gemm_q8_rows_kernel: the last three shapes)
@pytest.mark.parametrize("M,N,K", [(300, 384, 384), (128, 128, 128), (1, 1536, 384), (517, 384, 1536),
                                   (4500, 384, 384), (4100, 1152, 384), (4224, 1536, 384)])
@pytest.mark.parametrize("per_channel,unsigned", [(False, True), (True, False), (True, True)])
def test_operators_match_the_onnx_definitions_exactly(diag_lib, M, N, K, per_channel, unsigned):
    rng = np.random.default_rng(M * 7 + N + K + per_channel + 2 * unsigned)
    A = (rng.standard_normal((M, K)) * rng.choice([0.3, 1.0, 4.0], size=(M, 1))).astype(np.float32)
    A[rng.integers(0, M), rng.integers(0, K)] = 9.5   # an outlier sets the range, as in real activations
    Wf = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    W, d, sc = quantize_matrix(Wf, per_channel, unsigned)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32)
    got, xq, xp, acc = run_q8(diag_lib, 2, A, W, sc, bias, resid)
    q, xs, xz = dynamic_quantize(A)
    assert xp[0] == xs and int(xp[1]) == xz
    assert np.array_equal(xq, q)                                             # DynamicQuantizeLinear, byte for byte
    want_acc = (q.astype(np.int64) - xz) @ d.T                               # MatMulInteger
    assert np.array_equal(acc.astype(np.int64), want_acc)
    want = (want_acc.astype(np.float32) * (xs * sc)[None, :].astype(np.float32)).astype(np.float32)
    want = ((want + bias[None, :]).astype(np.float32) + resid).astype(np.float32)   # Cast, Mul, Add(bias), + residual
    assert np.array_equal(got, want)
    # plain store and the two split-form stores (f32-class: one split round trip; the GELU is the kernels' own erf)
    base = (want_acc.astype(np.float32) * (xs * sc)[None, :].astype(np.float32) + bias[None, :]).astype(np.float32)
    assert np.array_equal(run_q8(diag_lib, 0, A, W, sc, bias)[0], base)
    np.testing.assert_allclose(run_q8(diag_lib, 4, A, W, sc, bias)[0], base, rtol=3e-7, atol=1e-9)
    from scipy.special import erf
    gelu = 0.5 * base.astype(np.float64) * (1.0 + erf(base.astype(np.float64) / np.sqrt(2.0)))
    np.testing.assert_allclose(run_q8(diag_lib, 1, A, W, sc, bias)[0], gelu, rtol=2e-6, atol=2e-7)


@pytest.mark.parametrize("M,N,K", [(300, 1536, 384), (77, 128, 128), (4500, 1536, 384)])
def test_ffn_up_leaves_requantised(diag_lib, M, N, K):
    """FFN-up -> FFN-down: GELU(x W^T + b) is quantised again for the next Linear; the kernel computes the product twice
    (range pass, store pass) and never writes the f32 tensor.  Its bytes against DynamicQuantizeLinear of the numpy GELU:
    the kernels' own erf is 1.2e-7 off the exact one, so a value that sits on a rounding boundary may land on the other
    side — a handful of bytes, by one step."""
    from scipy.special import erf

    rng = np.random.default_rng(M + N)
    A = (rng.standard_normal((M, K)) * 1.5).astype(np.float32)
    W, d, sc = quantize_matrix((rng.standard_normal((N, K)) * 0.05).astype(np.float32), True, True)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    C_ = np.empty((M, N), np.float32)
    xp = np.empty(4, np.float32)
    rows = np.empty((M, N), np.int32)
    _lib.check_diag(diag_lib.cs_debug_gemm_q8(0, 5, 0, A.ctypes.data_as(f32p), W.ctypes.data_as(f32p), sc.ctypes.data_as(f32p),
                                        bias.ctypes.data_as(f32p), None, C_.ctypes.data_as(f32p), M, N, K, None,
                                        xp.ctypes.data_as(f32p), rows.ctypes.data_as(C.POINTER(C.c_int32))))
    q, xs, xz = dynamic_quantize(A)
    assert xp[0] == xs and int(xp[1]) == xz
    y = ((q.astype(np.int64) - xz) @ d.T).astype(np.float32) * (xs * sc)[None, :].astype(np.float32) + bias[None, :]
    g = (0.5 * y.astype(np.float64) * (1.0 + erf(y.astype(np.float64) / np.sqrt(2.0)))).astype(np.float32)
    gq, gs, gz = dynamic_quantize(g)
    assert abs(float(xp[2]) - float(gs)) <= 2e-6 * float(gs) and int(xp[3]) == gz
    diff = np.abs(C_.astype(np.int64) - gq.astype(np.int64))
    assert diff.max() <= 1 and (diff != 0).mean() < 2e-3
    assert np.array_equal(rows.reshape(-1)[:M], C_.astype(np.int64).sum(axis=1))   # the row sums the next product needs


@pytest.mark.parametrize("M,N,K,epi,a_split", [(16, 1152, 384, 4, 4), (9, 384, 384, 2, 5), (200, 1536, 384, 1, 4),
                                               (33, 384, 1536, 2, 5), (1, 384, 384, 0, 4)])
def test_few_rows_kernel_is_one_launch_with_the_same_bits(diag_lib, M, N, K, epi, a_split):
    """Query-side forwards run one launch per Linear (gemm_q8_skinny_kernel: range from the producer's pairs, the
    block's 16 rows quantised into LDS, K split over the waves): the same bytes and integers as the three-launch form."""
    rng = np.random.default_rng(M + N + K)
    A = (rng.standard_normal((M, K)) * 1.3).astype(np.float32)
    W, d, sc = quantize_matrix((rng.standard_normal((N, K)) * 0.05).astype(np.float32), True, False)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32) if epi == 2 else None
    got = run_q8(diag_lib, epi, A, W, sc, bias, resid, a_split=a_split)[0]
    ref = run_q8(diag_lib, epi, A, W, sc, bias, resid, a_split=a_split & 1)[0]
    assert np.array_equal(got, ref)


def test_row_block_products_quantise_their_own_rows(diag_lib):
    """From 4,096 rows a K = 384 Linear takes the f32-class tensor itself: each block of the product kernel quantises its
    128 rows on the way in (reciprocal multiply, the true division where the two could round apart).  Same bytes, same
    integers, so the same outputs bit for bit as the separate quantising pass."""
    from scipy.special import erf

    rng = np.random.default_rng(8)
    M, K = 4300, 384
    A = (rng.standard_normal((M, K)) * rng.choice([0.3, 1.0, 3.0], size=(M, 1))).astype(np.float32)
    for N, epi, a_split in ((1152, 4, 8), (384, 2, 9)):
        W, d, sc = quantize_matrix((rng.standard_normal((N, K)) * 0.05).astype(np.float32), True, True)
        bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
        resid = rng.standard_normal((M, N)).astype(np.float32)
        got = run_q8(diag_lib, epi, A, W, sc, bias, resid if epi == 2 else None, a_split=a_split)[0]
        ref = run_q8(diag_lib, epi, A, W, sc, bias, resid if epi == 2 else None, a_split=a_split & 1)[0]
        assert np.array_equal(got, ref)
        q, xs, xz = dynamic_quantize(split_round_trip(A) if a_split & 1 else A)
        base = (((q.astype(np.int64) - xz) @ d.T).astype(np.float32) * (xs * sc)[None, :].astype(np.float32) + bias[None, :]).astype(np.float32)
        if epi == 2:
            assert np.array_equal(got, (base + resid).astype(np.float32))
        else:
            np.testing.assert_allclose(got, base, rtol=3e-7, atol=1e-9)
    # FFN-up (two passes, re-quantised output) from the f32 tensor
    N = 1536
    W, d, sc = quantize_matrix((rng.standard_normal((N, K)) * 0.05).astype(np.float32), False, True)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    outs = []
    for a_split in (8, 0):
        C_ = np.empty((M, N), np.float32)
        xp = np.empty(4, np.float32)
        rows = np.empty((M, N), np.int32)
        _lib.check_diag(diag_lib.cs_debug_gemm_q8(0, 5, a_split, A.ctypes.data_as(f32p), W.ctypes.data_as(f32p), sc.ctypes.data_as(f32p),
                                            bias.ctypes.data_as(f32p), None, C_.ctypes.data_as(f32p), M, N, K, None,
                                            xp.ctypes.data_as(f32p), rows.ctypes.data_as(C.POINTER(C.c_int32))))
        outs.append((C_, xp.copy(), rows.reshape(-1)[:M].copy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1][2:], outs[1][1][2:]) and np.array_equal(outs[0][2], outs[1][2])


@pytest.mark.parametrize("M,N", [(300, 1152), (4500, 1536), (1, 128), (66000, 256), (513, 384)])
def test_slab_kernel_leaves_the_row_block_kernels_bits(diag_lib, M, N, monkeypatch):
    """At indexing batch sizes QKV and FFN-up run on gemm_q8_slab_kernel (a block owns 256 rows, W is the MFMA's first
    operand, the tile leaves from registers in 16-byte stores after half-wave exchanges): the same integers and the same
    f32 operations in the same order, so the same bits as the separate quantising pass + tile kernel — ragged slabs, n-tile
    ranges cut between blocks (few slabs) and blocks that walk several slabs (66,000 rows) included."""
    rng = np.random.default_rng(M + N)
    K = 384
    A = (rng.standard_normal((M, K)) * rng.choice([0.3, 1.0, 3.0], size=(M, 1))).astype(np.float32)
    W, d, sc = quantize_matrix((rng.standard_normal((N, K)) * 0.05).astype(np.float32), True, True)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    # (below 4,096 rows the comparison path is the tile kernel, whose store pass computes the GELU byte directly: the slab
    # kernel is put on its direct form too — the table form differs from it inside a few ulps of a rounding threshold)
    if M < 4096:
        monkeypatch.setenv("CS_Q8_GELU_TABLE", "0")
    # QKV: bias, split-f16 store
    got = run_q8(diag_lib, 4, A, W, sc, bias, None, a_split=16)[0]
    ref = run_q8(diag_lib, 4, A, W, sc, bias, None, a_split=0)[0]
    assert np.array_equal(got, ref)
    # FFN-up: range pass + re-quantising store pass (bytes, output parameters, row sums)
    outs = []
    for a_split in (16, 48, 0):   # 48 = 16 | 32: the store pass takes the rows the range pass quantised (s8) instead of quantising again
        C_ = np.empty((M, N), np.float32)
        xp = np.empty(4, np.float32)
        rows = np.empty((M, N), np.int32)
        _lib.check_diag(diag_lib.cs_debug_gemm_q8(0, 5, a_split, A.ctypes.data_as(f32p), W.ctypes.data_as(f32p), sc.ctypes.data_as(f32p),
                                            bias.ctypes.data_as(f32p), None, C_.ctypes.data_as(f32p), M, N, K, None,
                                            xp.ctypes.data_as(f32p), rows.ctypes.data_as(C.POINTER(C.c_int32))))
        outs.append((C_, xp.copy(), rows.reshape(-1)[:M].copy()))
    for o in outs[:2]:
        assert np.array_equal(o[1][2:], outs[2][1][2:])          # the output tensor's (scale, zero point)
        assert np.array_equal(o[2], outs[2][2])                  # the row sums FFN-down needs
        assert np.array_equal(o[0], outs[2][0])
        assert np.array_equal(o[2], o[0].astype(np.int64).sum(axis=1))


def _unit_rows(rng, L, units):
    """row_slot of a device batch of sequences of L positions: units = [(sequences, own padded length)], in order."""
    slots = []
    for u, (n, own) in enumerate(units):
        for _ in range(n):
            slots += [u | (0x80000000 if t >= own else 0) for t in range(L)]
    return np.array(slots, np.uint32)


def _quantize_with(x, lo, hi):
    scale = np.float32(1) if hi == lo else np.float32((np.float32(hi) - np.float32(lo)) / np.float32(255))
    zp = np.float32(np.rint(np.clip(np.float32(0) - np.float32(np.float32(lo) / scale), 0, 255)))
    return np.clip(np.rint((x / scale).astype(np.float32)) + zp, 0, 255).astype(np.uint8), scale, int(zp)


@pytest.mark.parametrize("L,units", [(50, [(30, 50), (2, 7), (40, 33), (18, 50)]),        # borders inside row blocks
                                     (128, [(8, 128), (8, 70), (16, 128), (4, 1)]),        # whole row blocks per unit
                                     (37, [(1, 37)] * 5 + [(110, 20), (1, 36)])])          # many units inside one row block
def test_row_block_products_over_several_units(diag_lib, L, units):
    """Queued calls share a device batch but stay their own quantisation units: the row-block products quantise every row
    with its OWN unit's (scale, zero point), a unit's range covers only the rows inside its own padded length, and the
    FFN-up range pass keeps the units' extremes apart — against numpy unit by unit: same bytes, same integers."""
    from scipy.special import erf

    rng = np.random.default_rng(L)
    slot = _unit_rows(rng, L, units)
    M, K = len(slot), 384
    assert M >= 4096
    U = len(units)
    su = slot & 0x7fffffff
    inc = (slot >> 31) == 0
    # every unit at its own magnitude (and rows outside a unit's own length larger still: they must not widen its range)
    A = (rng.standard_normal((M, K)) * rng.choice([0.2, 1.0, 4.0], size=U)[su][:, None]).astype(np.float32)
    A[~inc] *= np.float32(3)

    def run(epi, N, resid=None):
        W, d, sc = quantize_matrix((rng.standard_normal((N, K)) * 0.05).astype(np.float32), True, True)
        bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
        C_ = np.empty((M, N), np.float32)
        rp = np.empty((M, 4), np.float32)
        sums = np.empty(M, np.int32)
        _lib.check_diag(diag_lib.cs_debug_gemm_q8_units(0, epi, A.ctypes.data_as(f32p), W.ctypes.data_as(f32p), sc.ctypes.data_as(f32p),
                                                  bias.ctypes.data_as(f32p), None if resid is None else resid.ctypes.data_as(f32p),
                                                  C_.ctypes.data_as(f32p), M, N, K, slot.ctypes.data_as(C.POINTER(C.c_uint32)), U,
                                                  rp.ctypes.data_as(f32p), sums.ctypes.data_as(C.POINTER(C.c_int32))))
        return C_, rp, sums, d, sc, bias

    def base_of(src, d, sc, bias, rp):
        base = np.empty((M, d.shape[0]), np.float32)
        for u in range(U):
            rows = su == u
            own = rows & inc
            lo = min(np.float32(0), src[own].min()) if own.any() else np.float32(0)
            hi = max(np.float32(0), src[own].max()) if own.any() else np.float32(0)
            q, xs, xz = _quantize_with(src[rows], lo, hi)
            assert (rp[rows, 0] == xs).all() and (rp[rows, 1] == xz).all(), u
            base[rows] = ((q.astype(np.int64) - xz) @ d.T).astype(np.float32) * (xs * sc)[None, :].astype(np.float32) + bias[None, :]
        return base

    got, rp, _, d, sc, bias = run(4, 1152)                                   # QKV: f32 source -> split store
    np.testing.assert_allclose(got, base_of(A, d, sc, bias, rp), rtol=3e-7, atol=1e-9)
    resid = rng.standard_normal((M, 384)).astype(np.float32)
    got, rp, _, d, sc, bias = run(2, 384, resid)                             # out-proj: split source, + residual
    assert np.array_equal(got, (base_of(split_round_trip(A), d, sc, bias, rp) + resid).astype(np.float32))
    got, rp, sums, d, sc, bias = run(5, 1536)                                # FFN-up: GELU, quantised again per unit
    y = base_of(A, d, sc, bias, rp)
    gl = (0.5 * y.astype(np.float64) * (1.0 + erf(y.astype(np.float64) / np.sqrt(2.0)))).astype(np.float32)
    for u in range(U):
        rows = su == u
        own = rows & inc
        lo = min(np.float32(0), gl[own].min()) if own.any() else np.float32(0)
        hi = max(np.float32(0), gl[own].max()) if own.any() else np.float32(0)
        gq, gs, gz = _quantize_with(gl[rows], lo, hi)
        assert (np.abs(rp[rows, 2] - gs) <= 2e-6 * gs).all() and (rp[rows, 3] == gz).all(), u
        diff = np.abs(got[rows].astype(np.int64) - gq.astype(np.int64))
        assert diff.max() <= 1 and (diff != 0).mean() < 2e-3, (u, diff.max(), (diff != 0).mean())
    assert np.array_equal(sums, got.astype(np.int64).sum(axis=1))


def test_split_form_activations_quantise_like_their_f32_values(diag_lib):
    """Attention and GELU hand their outputs over in split-f16 form: the quantiser reads hi + lo / 2048."""
    rng = np.random.default_rng(5)
    M, N, K = 200, 384, 1536
    A = (rng.standard_normal((M, K)) * 2).astype(np.float32)
    W, d, sc = quantize_matrix((rng.standard_normal((N, K)) * 0.03).astype(np.float32), True, True)
    bias = np.zeros(N, np.float32)
    _, xq, xp, acc = run_q8(diag_lib, 0, A, W, sc, bias, a_split=1)
    q, xs, xz = dynamic_quantize(split_round_trip(A))
    assert xp[0] == xs and int(xp[1]) == xz and np.array_equal(xq, q)
    assert np.array_equal(acc.astype(np.int64), (q.astype(np.int64) - xz) @ d.T)


def test_degenerate_ranges_and_bad_blocks(diag_lib):
    M, N, K = 40, 128, 128
    W, d, sc = quantize_matrix(np.random.default_rng(1).standard_normal((N, K)).astype(np.float32) * 0.1, False, True)
    bias = np.arange(N, dtype=np.float32)
    # all-zero activations: hi == lo -> scale 1, zero point 0, the output is the bias
    got, xq, xp, _ = run_q8(diag_lib, 0, np.zeros((M, K), np.float32), W, sc, bias)
    assert xp[0] == 1.0 and xp[1] == 0.0 and not xq.any() and np.array_equal(got, np.tile(bias, (M, 1)))
    # all-negative and all-positive tensors: the range still includes zero
    for sign in (-1.0, 1.0):
        A = (sign * (1.0 + np.random.default_rng(2).random((M, K)))).astype(np.float32)
        _, xq, xp, _ = run_q8(diag_lib, 0, A, W, sc, bias)
        q, xs, xz = dynamic_quantize(A)
        assert xp[0] == xs and int(xp[1]) == xz == (255 if sign < 0 else 0) and np.array_equal(xq, q)
    # weights that are not multiples of their scales are refused, not silently re-quantised
    with pytest.raises(_lib.CsError, match="not a quantised matrix"):
        run_q8(diag_lib, 0, np.ones((M, K), np.float32), (W + np.float32(0.37) * sc[:, None]).astype(np.float32), sc, bias)


def small_cfg(pooling, layers=2):
    return BertConfig(vocab_size=1500, hidden=384, layers=layers, heads=12, intermediate=1536, max_position=64, pooling=pooling)


@pytest.mark.parametrize("per_channel,unsigned", [(False, True), (True, False), (True, True)])
def test_one_quantised_layer_is_the_oracles_except_for_flipped_bytes(gpu_lib, oracle, per_channel, unsigned):
    """One layer = four quantised Linears in a row.  Wherever no activation byte flips between the two f32-class
    evaluations the hidden states agree to f32 rounding; a flipped byte moves its own token row by ~1e-3.  Measured:
    0.6-1 % of the rows carry a flip."""
    from codesearch_amd import FastEmbedder, ModelType

    cfg = small_cfg(POOL_MEAN, layers=1)
    params, wscale = quantize_linear_weights(cfg, synth_params(cfg, 11), per_channel=per_channel, unsigned=unsigned)
    assert wscale.shape == (cfg.layers, quant_columns(cfg))
    ids, mask = synth_token_batch(cfg, 4, 24, 48, True)
    emb = FastEmbedder(ModelType.AllMiniLML6V2Q, config=cfg, params=params, wscale=wscale)
    got = emb.embed_ids(ids, mask)
    hid = emb.last_hidden(ids.size).reshape(ids.shape + (cfg.hidden,))
    want = oracle.bert_forward(cfg, params, ids, mask, wscale=wscale, want_hidden=True)
    f32_graph = oracle.bert_forward(cfg, params, ids, mask, want_hidden=True)
    valid = mask.astype(bool)
    err = np.abs(hid[valid] - want["hidden"][valid])
    assert np.median(err) < 5e-7
    assert (err.max(axis=1) > 1e-5).mean() < 0.04          # rows with a flipped byte
    assert err.max() < 2e-2 and np.abs(got - want["pooled"]).max() < 1e-3
    # not re-quantising the activations is a different function: every row moves, by thousands of times more
    assert np.median(np.abs(f32_graph["hidden"][valid] - want["hidden"][valid])) > 1e-3
    emb.close()


def test_activations_beyond_the_f16_range_degrade_instead_of_failing(gpu_lib, oracle):
    """onnxruntime embeds whatever the activations are (/root/reference/src/embed/embedder.rs:286-289); this mode hands Q / K / V
    and the attention output over in split-f16 form, which ends at 65504.  A value-bias block of 1e5 trips that: the
    mini-batch is then run again as the f32 graph of the dequantised weights (the same model without the 8-bit rounding of
    the activations) and counted — not refused.  The result against the oracle's f32 evaluation of those weights, and a
    mini-batch that stays in range against the quantised oracle as always."""
    from codesearch_amd import FastEmbedder, ModelType
    from codesearch_amd.bert_params import to_state_dict, from_state_dict

    cfg = small_cfg(POOL_MEAN)
    params, wscale = quantize_linear_weights(cfg, synth_params(cfg, 31), per_channel=False, unsigned=True)
    sd = to_state_dict(cfg, params)
    sd["encoder.layer.0.attention.self.value.bias"] = sd["encoder.layer.0.attention.self.value.bias"] + np.float32(1.0e5)
    big = from_state_dict(cfg, sd)
    ids, mask = synth_token_batch(cfg, 6, 16, 40, True)
    emb = FastEmbedder(ModelType.AllMiniLML6V2Q, config=cfg, params=big, wscale=wscale)
    assert emb.gemm_mode() == "q8"
    got = emb.embed_ids(ids, mask)                     # (before: CS_ERR_UNSUPPORTED "left the f16 range")
    _, f32_forwards, fallbacks = emb.debug_counters()
    assert fallbacks == 1 and f32_forwards == 1
    want = oracle.bert_forward(cfg, big, ids, mask)["pooled"]          # the f32 graph of the dequantised weights
    assert np.isfinite(got).all() and np.abs(got - want).max() < 1e-4
    emb.close()
    # the same weights without the block: no fallback, the quantised graph
    emb = FastEmbedder(ModelType.AllMiniLML6V2Q, config=cfg, params=params, wscale=wscale)
    got = emb.embed_ids(ids, mask)
    assert emb.debug_counters()[2] == 0
    want = oracle.bert_forward(cfg, params, ids, mask, wscale=wscale)["pooled"]
    assert np.abs(got - want).max() < 3e-3
    emb.close()


@pytest.mark.parametrize("pooling", [POOL_MEAN, POOL_CLS])
@pytest.mark.parametrize("per_channel,unsigned", [(False, True), (True, False)])
def test_quantised_forward_against_the_oracle(gpu_lib, oracle, pooling, per_channel, unsigned):
    """Two layers: a flipped byte in layer 1 reaches every token of its sequence through attention, and one that sits
    on a tensor's extreme value moves that tensor's scale — dynamic quantisation is discontinuous, in the reference's
    runtime as here.  The bar is the average distance, against what ignoring the activation quantisation would cost."""
    from codesearch_amd import FastEmbedder, ModelType

    cfg = small_cfg(pooling)
    params, wscale = quantize_linear_weights(cfg, synth_params(cfg, 11), per_channel=per_channel, unsigned=unsigned)
    ids, mask = synth_token_batch(cfg, 4, 24, 48, True)
    emb = FastEmbedder(ModelType.AllMiniLML6V2Q, config=cfg, params=params, wscale=wscale)
    got = emb.embed_ids(ids, mask)
    want = oracle.bert_forward(cfg, params, ids, mask, wscale=wscale)["pooled"]
    f32_graph = oracle.bert_forward(cfg, params, ids, mask)["pooled"]
    err, noise = np.abs(got - want), np.abs(f32_graph - want)
    assert err.max() < 3e-3 and (got * want).sum(1).min() > 0.99999
    assert err.mean() < 0.5 * noise.mean(), (err.mean(), noise.mean())
    np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
    # the f32 graph of the same (quantised) weights is still there on request, and is the other thing
    emb.set_gemm_mode("split")
    np.testing.assert_allclose(emb.embed_ids(ids, mask), f32_graph, atol=2e-5)
    emb.set_gemm_mode("q8")
    assert np.array_equal(emb.embed_ids(ids, mask), got)   # deterministic: integer atomics, fixed summation orders
    emb.close()
    # a model that is not quantised has no such mode
    plain = FastEmbedder(ModelType.BGESmallENV15, config=cfg, seed=3)
    with pytest.raises(_lib.CsError, match="needs a quantised model"):
        plain.set_gemm_mode("q8")
    plain.close()


def test_a_call_is_one_tensor(gpu_lib, oracle):
    """DynamicQuantizeLinear sees the whole call: the same text embeds differently beside an outlier sequence, exactly
    as it does in the reference's runtime; batches are `batch` consecutive rows in the caller's order."""
    from codesearch_amd import FastEmbedder, ModelType

    cfg = small_cfg(POOL_MEAN)
    params, wscale = quantize_linear_weights(cfg, synth_params(cfg, 2), per_channel=False, unsigned=True)
    ids, mask = synth_token_batch(cfg, 9, 6, 32, True)
    emb = FastEmbedder(ModelType.AllMiniLML6V2Q, config=cfg, params=params, wscale=wscale)
    whole = emb.embed_ids(ids, mask, batch_size=6)
    halves = emb.embed_ids(ids, mask, batch_size=3)
    for name, got, parts in (("one call", whole, [slice(0, 6)]), ("two calls", halves, [slice(0, 3), slice(3, 6)])):
        want = np.concatenate([oracle.bert_forward(cfg, params, ids[p], mask[p], wscale=wscale)["pooled"] for p in parts])
        assert np.abs(got - want).max() < 3e-3, name
    assert np.abs(whole - halves).max() > 1e-5   # the call boundary matters in this mode (and only in this mode)
    emb.close()


@pytest.mark.parametrize("qdtype_name,per_channel,style,rel", [("UINT8", False, "quantized", "onnx/model_quantized.onnx"),
                                                               ("INT8", True, "quantized", "onnx/model_quantized.onnx"),
                                                               ("INT8", False, "optimized_quantized", "model_optimized.onnx")])
def test_quantised_model_directory(gpu_lib, oracle, tmp_path, qdtype_name, per_channel, style, rel):
    """What fastembed's cache holds for a *Q registry entry (the reference's default model among them): config.json and
    onnx/model_quantized.onnx as onnxruntime's quantize_dynamic writes it.  FastEmbedder.from_dir must come up in the
    dynamic-quantisation mode and embed as the oracle's quantised forward does on the block and scales read back from
    the file; CS_ENCODER_QUANT=0 keeps the f32 graph of the same weights."""
    import json
    import os

    from codesearch_amd import FastEmbedder
    from codesearch_amd.bert_params import to_state_dict
    from tests import onnx_writer
    from tests.test_model_files import load_onnx_q

    cfg = small_cfg(POOL_MEAN)
    sd = to_state_dict(cfg, synth_params(cfg, 21))
    config = {"model_type": "bert", "vocab_size": cfg.vocab_size, "hidden_size": 384, "num_hidden_layers": cfg.layers,
              "num_attention_heads": 12, "intermediate_size": 1536, "max_position_embeddings": cfg.max_position,
              "type_vocab_size": 2, "layer_norm_eps": 1e-12, "hidden_act": "gelu"}
    cache = tmp_path / "models--Xenova--all-MiniLM-L6-v2" / "snapshots" / "abc"
    (cache / "onnx").mkdir(parents=True)
    (cache / "config.json").write_text(json.dumps(config))
    path = cache / rel   # (the third case: the BGE-small *Q entry's file, through onnxruntime's transformer optimiser)
    path.write_bytes(onnx_writer.bert_onnx(sd, cfg.layers, style, qdtype=getattr(onnx_writer, qdtype_name),
                                           per_channel=per_channel, quantize_tables=True))
    params, wscale, quantized = load_onnx_q(gpu_lib, path, cfg)
    assert quantized == 1
    ids, mask = synth_token_batch(cfg, 6, 16, 40, True)
    emb = FastEmbedder.from_dir(str(cache), pooling=POOL_MEAN)
    assert emb.gemm_mode() == "q8"
    got = emb.embed_ids(ids, mask)
    want = oracle.bert_forward(cfg, params, ids, mask, wscale=wscale)["pooled"]
    f32_graph = oracle.bert_forward(cfg, params, ids, mask)["pooled"]
    err, noise = np.abs(got - want), np.abs(f32_graph - want)
    assert err.max() < 3e-3 and err.mean() < 0.5 * noise.mean(), (err.max(), err.mean(), noise.mean())
    emb.close()
    os.environ["CS_ENCODER_QUANT"] = "0"
    try:
        emb = FastEmbedder.from_dir(str(cache), pooling=POOL_MEAN)
        assert emb.gemm_mode() == "split"
        np.testing.assert_allclose(emb.embed_ids(ids, mask), f32_graph, atol=2e-5)
        emb.close()
    finally:
        del os.environ["CS_ENCODER_QUANT"]


def test_texts_and_queued_submissions_are_quantised_per_reference_call(gpu_lib, oracle):
    """From strings a call tensor is `batch` CONSECUTIVE texts padded to their longest (fastembed's batches: no length
    grouping, no token-budget batches in this mode); through the queue it is one submission (the reference hands ORT one
    32-chunk slice at a time, /root/reference/src/embed/batch.rs:84-115) — coalescing submissions into one device batch
    would change every range."""
    import json
    import os

    from codesearch_amd import FastEmbedder, ModelType
    from codesearch_amd.tokenizer import BertWordPieceTokenizer

    G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "tokenizer_golden.json")))
    tok = BertWordPieceTokenizer(G["vocab"])
    cfg = BertConfig(vocab_size=len(G["vocab"]), hidden=384, layers=2, heads=12, intermediate=1536, max_position=128,
                     pooling=POOL_MEAN)
    params, wscale = quantize_linear_weights(cfg, synth_params(cfg, 5), per_channel=True, unsigned=True)
    emb = FastEmbedder(ModelType.AllMiniLML6V2Q, config=cfg, params=params, wscale=wscale, tokenizer=tok)
    texts = ["fn main() { println!(\"hello world\"); }", "def calculate(a, b): return a", "struct", "x" * 150,
             "impl Display for Point { fn fmt(&self, f: &mut Formatter) -> Result { write!(f, \"({}, {})\", self.x, self.y) } }",
             "", "let v: Vec<u32> = (0..10).collect();", "class Foo(Bar): pass", "SELECT * FROM chunks WHERE id = 7",
             "// comment only", "return"]

    def per_call(groups):
        out = []
        for g in groups:
            ids, mask = tok.encode_batch(g)
            out.append(oracle.bert_forward(cfg, params, ids, mask, wscale=wscale)["pooled"])
        return np.concatenate(out)

    got = np.stack(emb.embed_batch_chunked(texts, 4))
    want = per_call([texts[i:i + 4] for i in range(0, len(texts), 4)])
    assert np.abs(got - want).max() < 3e-3 and np.abs(got - want).mean() < 1e-4
    # grouped differently the same texts embed differently: the unit matters, and it is the caller's
    assert np.abs(got - per_call([texts[:8], texts[8:]])).mean() > 2 * np.abs(got - want).mean()
    # the queue: three submissions, one wait each, each its own tensor whatever else is queued
    subs = [texts[:5], texts[5:6], texts[6:]]
    tickets = [emb.submit_texts(s) for s in subs]
    for s, t in zip(reversed(subs), reversed(tickets)):
        e = np.abs(emb.wait(t) - per_call([s]))
        assert e.max() < 3e-3 and e.mean() < 1e-4
    emb.close()


def test_queued_submissions_share_a_device_batch_and_keep_their_own_ranges(gpu_lib, oracle):
    """Several submissions embedded as ONE forward: every row carries its own call's quantisation range (and a call's
    rows beyond its own padded length stay out of that range), so each submission's embeddings are those of the call
    run alone — the throughput of the large batch without changing what a quantised model computes."""
    from codesearch_amd import FastEmbedder, ModelType

    cfg = small_cfg(POOL_MEAN)
    params, wscale = quantize_linear_weights(cfg, synth_params(cfg, 31), per_channel=False, unsigned=True)
    emb = FastEmbedder(ModelType.AllMiniLML6V2Q, config=cfg, params=params, wscale=wscale)
    rng = np.random.default_rng(3)
    subs = []
    for n, L in ((5, 40), (1, 12), (9, 64), (3, 25), (7, 33)):   # different sizes, different longest rows
        ids, mask = synth_token_batch(cfg, int(rng.integers(1, 1000)), n, L, True)
        ids[0, -1], mask[0, -1] = 102, 1                         # one full-length row: L is the call's padded length
        subs.append((ids, mask))
    emb.profile_read(reset=True)
    tickets = [emb.submit_ids(i, m) for i, m in subs]
    got = [emb.wait(t) for t in tickets]
    _, forwards = emb.profile_read()
    assert forwards == 1, forwards                               # 25 rows, five units, one device batch
    alone = []
    for (ids, mask), g in zip(subs, got):
        want = oracle.bert_forward(cfg, params, ids, mask, wscale=wscale)["pooled"]
        e = np.abs(g - want)
        assert e.max() < 3e-3 and e.mean() < 1.5e-4, (e.max(), e.mean())
        alone.append(emb.embed_ids(ids, mask))                   # the same call on its own: one unit, other kernels
    # sharing the batch is not what moves an embedding: against the call run alone the distance is the same flip noise,
    # and embedding one call's rows with ANOTHER call's range would be far outside it
    for g, a in zip(got, alone):
        assert np.abs(g - a).max() < 3e-3 and np.abs(g - a).mean() < 1.5e-4
    ids_all = np.zeros((25, 64), np.int32)
    mask_all = np.zeros((25, 64), np.int32)
    r = 0
    for ids, mask in subs:
        ids_all[r:r + len(ids), :ids.shape[1]] = ids
        mask_all[r:r + len(ids), :ids.shape[1]] = mask
        r += len(ids)
    one_tensor = emb.embed_ids(ids_all, mask_all)                # what ignoring the units would compute
    assert np.abs(one_tensor - np.concatenate(got)).mean() > 3 * np.abs(np.concatenate(got) - np.concatenate(alone)).mean()
    emb.close()


def test_queued_units_on_the_row_block_kernels(gpu_lib, oracle):
    """From 4,096 token rows a device batch of several units runs the one-unit path's kernels (per-row parameters on load,
    per-unit ranges from the producers' pairs, the two-pass FFN-up per unit): one forward, and the same bars against the
    oracle per submission as the general form is held to (its operators are compared with numpy unit by unit in
    test_row_block_products_over_several_units)."""
    from codesearch_amd import FastEmbedder, ModelType

    cfg = BertConfig(vocab_size=900, hidden=384, layers=2, heads=12, intermediate=1536, max_position=160, pooling=POOL_MEAN)
    params, wscale = quantize_linear_weights(cfg, synth_params(cfg, 41), per_channel=True, unsigned=True)
    emb = FastEmbedder(ModelType.AllMiniLML6V2Q, config=cfg, params=params, wscale=wscale)
    rng = np.random.default_rng(5)
    subs = []
    for n, L in ((20, 128), (1, 9), (10, 100), (12, 128), (3, 37)):      # 46 rows x 128 = 5,888 token rows, five units
        ids, mask = synth_token_batch(cfg, int(rng.integers(1, 1000)), n, L, True)
        ids[0, -1], mask[0, -1] = 102, 1
        subs.append((ids, mask))
    emb.profile_read(reset=True)
    tickets = [emb.submit_ids(i, m) for i, m in subs]
    got = [emb.wait(t) for t in tickets]
    _, forwards = emb.profile_read()
    assert forwards == 1, forwards
    for (ids, mask), g in zip(subs, got):
        want = oracle.bert_forward(cfg, params, ids, mask, wscale=wscale)["pooled"]
        e = np.abs(g - want)
        assert np.isfinite(g).all() and e.max() < 4e-3 and e.mean() < 2.5e-4, (ids.shape, e.max(), e.mean())
    emb.close()


def test_random_shapes_and_unit_mixes_stay_within_the_flip_noise(gpu_lib, oracle):
    """Shapes the fixed cases do not visit: one-token rows, a single row, batches around the kernels' tile and row-block
    thresholds, queued units of very different lengths (so most of a unit's rows lie beyond its own padded length)."""
    from codesearch_amd import FastEmbedder, ModelType

    cfg = BertConfig(vocab_size=900, hidden=384, layers=2, heads=12, intermediate=1536, max_position=160, pooling=POOL_MEAN)
    params, wscale = quantize_linear_weights(cfg, synth_params(cfg, 77), per_channel=True, unsigned=True)
    emb = FastEmbedder(ModelType.AllMiniLML6V2Q, config=cfg, params=params, wscale=wscale)
    rng = np.random.default_rng(12)

    def batch(n, L):
        ids, mask = synth_token_batch(cfg, int(rng.integers(1, 10_000)), n, L, L > 2)
        return ids, mask

    def check(got, ids, mask, what):
        want = oracle.bert_forward(cfg, params, ids, mask, wscale=wscale)["pooled"]
        e = np.abs(got - want)
        assert np.isfinite(got).all() and e.max() < 4e-3 and e.mean() < 2.5e-4, (what, e.max(), e.mean())

    for n, L in ((1, 1), (1, 7), (3, 2), (2, 129), (33, 128), (40, 103), (64, 65)):   # 4,224 / 4,120 / 4,160 rows: row-block kernel
        ids, mask = batch(n, L)
        check(emb.embed_ids(ids, mask, batch_size=n), ids, mask, (n, L))
    for _ in range(3):
        subs = [batch(int(rng.integers(1, 12)), int(rng.choice([1, 3, 17, 64, 150]))) for _ in range(int(rng.integers(2, 7)))]
        tickets = [emb.submit_ids(i, m) for i, m in subs]
        for (ids, mask), t in zip(subs, tickets):
            check(emb.wait(t), ids, mask, ("queued", ids.shape))
    emb.close()


@pytest.mark.parametrize("hidden,heads,inter", [(768, 12, 3072), (1024, 16, 4096)])
def test_quantised_wider_models(gpu_lib, oracle, hidden, heads, inter):
    """hidden 768 / 1,024 (head_dim 64; K = 768 ... 4,096 in the products: the tile-per-block kernel, 24-bit zero-point
    arithmetic at its widest).  Wider rows carry more activation bytes each: 2-15 % of the rows hold a flipped one after a
    single layer and, in about one input in four, one of them is a tensor's extreme, which moves that tensor's scale and
    with it every row by ~2e-3 (benchmarks/q8_wide_probe.py) — so the bar is the distance against what ignoring the
    activation quantisation costs, as for the two-layer model."""
    from codesearch_amd import FastEmbedder, ModelType

    cfg = BertConfig(vocab_size=600, hidden=hidden, layers=1, heads=heads, intermediate=inter, max_position=64, pooling=POOL_CLS)
    params, wscale = quantize_linear_weights(cfg, synth_params(cfg, 41), per_channel=True, unsigned=True)
    emb = FastEmbedder(ModelType.BGEBaseENV15, config=cfg, params=params, wscale=wscale)
    assert emb.gemm_mode() == "q8"
    clean = 0
    for iseed in (14, 55, 56):
        ids, mask = synth_token_batch(cfg, iseed, 20, 48, True)
        got = emb.embed_ids(ids, mask)
        hid = emb.last_hidden(ids.size).reshape(ids.shape + (hidden,))
        want = oracle.bert_forward(cfg, params, ids, mask, wscale=wscale, want_hidden=True)
        f32_graph = oracle.bert_forward(cfg, params, ids, mask, want_hidden=True)
        valid = mask.astype(bool)
        err = np.abs(hid[valid] - want["hidden"][valid])
        noise = np.abs(f32_graph["hidden"][valid] - want["hidden"][valid])
        assert err.mean() < 0.5 * noise.mean() and np.abs(got - want["pooled"]).max() < 5e-3, (iseed, err.mean(), noise.mean())
        clean += int(np.median(err) < 1e-6)
    assert clean >= 1   # where no extreme moved, the rows agree to f32 rounding
    emb.close()


def test_slab_kernels_inside_a_forward(gpu_lib, oracle, tmp_path):
    """From 8,192 token rows a quantised forward runs QKV and FFN-up on gemm_q8_slab_kernel (the store pass taking the rows
    the range pass quantised).  A 320 x 40-token call (12,800 rows, two layers): against the quantised oracle at the model
    level's usual bar, and BIT FOR BIT against the same call on the row-block kernels (CS_Q8_SLAB_MIN_M=0 — a laboratory
    knob read once per process: a child process on the diagnostic library)."""
    import os
    import subprocess
    import sys

    from codesearch_amd import FastEmbedder, ModelType, _lib

    cfg = small_cfg(POOL_MEAN)
    params, wscale = quantize_linear_weights(cfg, synth_params(cfg, 41), per_channel=False, unsigned=True)
    ids, mask = synth_token_batch(cfg, 42, 320, 40, True)
    emb = FastEmbedder(ModelType.AllMiniLML6V2Q, config=cfg, params=params, wscale=wscale)
    got = emb.embed_ids(ids, mask, batch_size=320)
    emb.close()
    want = oracle.bert_forward(cfg, params, ids, mask, wscale=wscale)["pooled"]
    err = np.abs(got - want)
    assert err.max() < 3e-3 and np.median(err) < 2e-5, (err.max(), np.median(err))
    code = (
        "import numpy as np, sys\n"
        "from codesearch_amd import FastEmbedder, ModelType\n"
        "from codesearch_amd.bert_params import POOL_MEAN, BertConfig, quantize_linear_weights, synth_params, synth_token_batch\n"
        "cfg = BertConfig(vocab_size=1500, hidden=384, layers=2, heads=12, intermediate=1536, max_position=64, pooling=POOL_MEAN)\n"
        "params, wscale = quantize_linear_weights(cfg, synth_params(cfg, 41), per_channel=False, unsigned=True)\n"
        "ids, mask = synth_token_batch(cfg, 42, 320, 40, True)\n"
        "emb = FastEmbedder(ModelType.AllMiniLML6V2Q, config=cfg, params=params, wscale=wscale)\n"
        "np.save(sys.argv[1], emb.embed_ids(ids, mask, batch_size=320))\n")
    out = str(tmp_path / "rowblock.npy")
    env = dict(os.environ, CS_Q8_SLAB_MIN_M="0", CS_LIBCSGPU=_lib.DIAG_LIB_PATH)
    subprocess.run([sys.executable, "-c", code, out], check=True, env=env, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert np.load(out).tobytes() == got.tobytes()


@pytest.mark.parametrize("B,L,ragged", [(1, 16, False), (1, 5, False), (2, 8, True), (1, 1, False), (3, 5, True), (1, 12, False)])
@pytest.mark.parametrize("pooling", [POOL_MEAN, POOL_CLS])
def test_one_short_query_folds_its_layernorms_into_the_products(gpu_lib, oracle, monkeypatch, B, L, ragged, pooling):
    """Up to 16 token rows of a 384-wide quantised model (one short query — `codesearch search` on the reference's default
    model): the two LayerNorms of a layer run as the prologues of the products that read them (Q8_SRC_LN: the block's 16
    rows are the whole call tensor, so it knows its range), five launches per layer instead of seven.  The same arithmetic
    (layernorm_kernel's), so the SAME BITS as the chain with LayerNorm launches (CS_Q8_SKINNY_LN=0), and the quantised
    oracle's embedding at the model level's bar."""
    from codesearch_amd import FastEmbedder, ModelType

    cfg = small_cfg(pooling, layers=3)
    params, wscale = quantize_linear_weights(cfg, synth_params(cfg, 61), per_channel=False, unsigned=True)
    ids, mask = synth_token_batch(cfg, 62 + B * 8 + L, B, L, ragged)
    emb = FastEmbedder(ModelType.AllMiniLML6V2Q, config=cfg, params=params, wscale=wscale)
    assert emb.gemm_mode() == "q8"
    monkeypatch.setenv("CS_Q8_SKINNY_LN", "0")
    chain = emb.embed_ids(ids, mask, batch_size=B)
    monkeypatch.setenv("CS_Q8_SKINNY_LN", "1")
    folded = emb.embed_ids(ids, mask, batch_size=B)
    assert folded.tobytes() == chain.tobytes(), float(np.abs(folded - chain).max())
    assert emb.embed_ids(ids, mask, batch_size=B).tobytes() == folded.tobytes()
    emb.close()
    want = oracle.bert_forward(cfg, params, ids, mask, wscale=wscale)["pooled"]
    err = np.abs(folded - want)
    assert err.max() < 3e-3, (err.max(), np.median(err))


def test_a_query_and_its_variants_on_wide_blocks(gpu_lib, oracle, tmp_path):
    """From 128 token rows the few-rows quantised products of the wide layers (QKV, FFN-up) run on 16 x 64 blocks (a wave =
    one column tile over all of K; gemm_q8_skinny_kernel WIDE).  Nine and twelve 16-token sequences: the quantised oracle's
    embedding at the model level's bar, and BIT FOR BIT the embedding of the 16 x 16 blocks (CS_Q8_SKINNY_WIDE_MIN_M=0 — a
    laboratory knob read once per process: a child process on the diagnostic library)."""
    import os
    import subprocess
    import sys

    from codesearch_amd import FastEmbedder, ModelType, _lib

    cfg = small_cfg(POOL_MEAN, layers=3)
    params, wscale = quantize_linear_weights(cfg, synth_params(cfg, 71), per_channel=False, unsigned=True)
    outs = {}
    for B in (9, 12):
        ids, mask = synth_token_batch(cfg, 72 + B, B, 16, True)
        emb = FastEmbedder(ModelType.AllMiniLML6V2Q, config=cfg, params=params, wscale=wscale)
        outs[B] = emb.embed_ids(ids, mask, batch_size=B)
        emb.close()
        want = oracle.bert_forward(cfg, params, ids, mask, wscale=wscale)["pooled"]
        assert np.abs(outs[B] - want).max() < 3e-3
    code = (
        "import numpy as np, sys\n"
        "from codesearch_amd import FastEmbedder, ModelType\n"
        "from codesearch_amd.bert_params import POOL_MEAN, BertConfig, quantize_linear_weights, synth_params, synth_token_batch\n"
        "cfg = BertConfig(vocab_size=1500, hidden=384, layers=3, heads=12, intermediate=1536, max_position=64, pooling=POOL_MEAN)\n"
        "params, wscale = quantize_linear_weights(cfg, synth_params(cfg, 71), per_channel=False, unsigned=True)\n"
        "for B in (9, 12):\n"
        "    ids, mask = synth_token_batch(cfg, 72 + B, B, 16, True)\n"
        "    emb = FastEmbedder(ModelType.AllMiniLML6V2Q, config=cfg, params=params, wscale=wscale)\n"
        "    np.save(sys.argv[1] + str(B) + '.npy', emb.embed_ids(ids, mask, batch_size=B))\n"
        "    emb.close()\n")
    env = dict(os.environ, CS_Q8_SKINNY_WIDE_MIN_M="0", CS_LIBCSGPU=_lib.DIAG_LIB_PATH)
    subprocess.run([sys.executable, "-c", code, str(tmp_path / "narrow")], check=True, env=env,
                   cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for B in (9, 12):
        assert np.load(str(tmp_path / "narrow") + f"{B}.npy").tobytes() == outs[B].tobytes()


@pytest.mark.parametrize("B,L", [(256, 16), (264, 16), (320, 40), (512, 64), (1024, 64)])
def test_layernorm_fused_products_repeat_their_bits(gpu_lib, oracle, B, L):
    """A race screen for the LayerNorm-fused products (gemm_q8_ln_kernel: weight stages by LDS-DMA behind COUNTED vmcnt waits
    and bare barriers, fragment reads in flight across them, MI355X guide: "place reads by the vmcnt / barrier count, never
    by clean runs").  Token-row counts with one 128-row group per block (4,096), a ragged last group (4,224), several
    groups per block (32,768; 65,536 = two per block on 256 CUs): the same call eight times must leave the same bytes
    (a stage read before it landed shows as a run that differs), and the first run meets the quantised oracle at the
    model level's bar.  That the bits are the RIGHT ones — the kernel alone against float64 inside a derived bound, every
    source, ragged groups, several groups per block — is tests/test_gpu_q8_ln.py."""
    from codesearch_amd import FastEmbedder, ModelType

    cfg = small_cfg(POOL_MEAN)
    params, wscale = quantize_linear_weights(cfg, synth_params(cfg, 51), per_channel=False, unsigned=True)
    ids, mask = synth_token_batch(cfg, 52 + B, B, L, True)
    emb = FastEmbedder(ModelType.AllMiniLML6V2Q, config=cfg, params=params, wscale=wscale)
    assert emb.gemm_mode() == "q8"
    first = emb.embed_ids(ids, mask, batch_size=B)
    for _ in range(7):
        assert emb.embed_ids(ids, mask, batch_size=B).tobytes() == first.tobytes()
    emb.close()
    if B * L <= 16384:  # (the C oracle's forward is seconds per 10k token rows)
        want = oracle.bert_forward(cfg, params, ids, mask, wscale=wscale)["pooled"]
        err = np.abs(first - want)
        assert err.max() < 3e-3 and np.median(err) < 2e-5, (err.max(), np.median(err))


def test_search_results_are_stable_under_quantisation_noise(gpu_lib, oracle):
    """What a USER of the default (quantised) model sees: 20,480 chunks and 64 queries embedded in the
    dynamic-quantisation mode by the GPU and by the quantised oracle (the same 256-row call tensors), each side searched
    for its top-10.  The two evaluations disagree on a few activation bytes per tensor, so an embedding moves by up to
    `delta` (L2; measured here, asserted below its bound); a unit-vector cosine then moves by at most delta_q + delta_x.
    The bar: every id the two top-10 lists do not share sits within that band of the oracle's 10th cosine — nothing outside
    the noise band ever changes rank — planted near-duplicates are found first by both, and the lists agree on at least 9
    of 10 ids on average."""
    from codesearch_amd import FastEmbedder, ModelType, VectorStore

    cfg = BertConfig(vocab_size=2048, hidden=384, layers=2, heads=12, intermediate=1536, max_position=64, pooling=POOL_MEAN)
    params, wscale = quantize_linear_weights(cfg, synth_params(cfg, 31), per_channel=False, unsigned=True)
    N, L, Q, K, CALL = 20480, 16, 64, 10, 256
    ids, mask = synth_token_batch(cfg, 77, N, L, False)
    rng = np.random.default_rng(5)
    planted = rng.choice(N, Q, replace=False)
    qids, qmask = ids[planted].copy(), mask[planted].copy()
    for i in range(Q):  # a query = its chunk with three inner tokens replaced
        for p in rng.choice(np.arange(1, L - 1), 3, replace=False):
            qids[i, p] = int(rng.integers(1000, cfg.vocab_size))
    emb = FastEmbedder(ModelType.AllMiniLML6V2Q, config=cfg, params=params, wscale=wscale)
    assert emb.gemm_mode() == "q8"
    g_rows = emb.embed_ids(ids, mask, batch_size=CALL)
    g_q = emb.embed_ids(qids, qmask, batch_size=Q)
    emb.close()
    o_rows = np.concatenate([oracle.bert_forward(cfg, params, ids[i:i + CALL], mask[i:i + CALL], wscale=wscale)["pooled"]
                             for i in range(0, N, CALL)])
    o_q = oracle.bert_forward(cfg, params, qids, qmask, wscale=wscale)["pooled"]
    d_rows = np.linalg.norm(g_rows - o_rows, axis=1)
    d_q = np.linalg.norm(g_q - o_q, axis=1)
    # the flip noise: median row far below its worst (most rows carry no flipped byte that matters)
    assert d_rows.max() < 1e-2 and np.median(d_rows) < 1e-3, (d_rows.max(), np.median(d_rows))
    assert np.abs(g_rows - o_rows).max() < 3e-3
    store = VectorStore(None, cfg.hidden, device=0)
    store.insert_embeddings(g_rows)
    store.build_index()
    g_cos, g_ids, cnt = store.search_raw(g_q, K)
    assert (cnt == K).all()
    o_cos_all = o_q @ o_rows.T                                     # [Q, N] oracle-side cosines of the oracle's embeddings
    shared, worst_excess, top1_same = 0, 0.0, 0
    for i in range(Q):
        o_ids = np.lexsort((np.arange(N), -o_cos_all[i]))[:K]       # (cosine desc, id asc)
        kth = o_cos_all[i, o_ids[-1]]
        band = d_q[i] + d_rows.max()
        gi, oi = set(g_ids[i].tolist()), set(o_ids.tolist())
        shared += len(gi & oi)
        for r in gi ^ oi:                                           # in one list only: inside the noise band of the k-th cosine
            worst_excess = max(worst_excess, abs(o_cos_all[i, r] - kth) - 2 * band)
        top1_same += int(g_ids[i][0] == o_ids[0])
        # the planted chunk is found by both whenever its margin over the runner-up exceeds the band
        margin = o_cos_all[i, planted[i]] - np.partition(np.delete(o_cos_all[i], planted[i]), -1)[-1]
        if margin > 2 * band:
            assert g_ids[i][0] == planted[i] == o_ids[0], (i, margin, band)
    assert worst_excess <= 0.0, worst_excess
    assert shared >= 0.9 * Q * K, shared / (Q * K)
    print(f"q8 top-{K} stability over {N} chunks, {Q} queries: {shared / (Q * K):.4f} of ids shared, top-1 equal {top1_same}/{Q}, "
          f"row noise L2 median {np.median(d_rows):.2e} max {d_rows.max():.2e}, query noise max {d_q.max():.2e}")
    store.close()
