"""The host half of the reranker (csrc/rerank_host.cpp: the ordering of NeuralReranker::rerank and the blend of
rerank_and_blend, src/rerank/neural.rs:77-121 of the reference) against a float32 numpy statement of the same lines, and the
score head's loader (cs_rerank_head_from_safetensors, cs_reranker_create_from_dir's refusals) on checkpoints written here.
CPU only: none of this touches a device."""
import ctypes as C
import json

import numpy as np
import pytest

from codesearch_amd import _lib, rerank
from codesearch_amd.bert_params import POOL_CLS, BertConfig, synth_params, to_state_dict
from codesearch_amd.search import rerank_step, rerank_take_count
from codesearch_amd.vector_store import SearchResult

f32 = np.float32


def sigmoid32(x):
    return f32(1.0) / (f32(1.0) + np.exp(-np.asarray(x, f32)))


def reference_blend(logits, rrf):
    """neural.rs:96-118 in float32: (index, blended) sorted by blended descending, stably from index order."""
    logits, rrf = np.asarray(logits, f32), np.asarray(rrf, f32)
    lo, hi = rrf.min(), rrf.max()
    rng = max(f32(hi - lo), f32(0.0001))
    blended = f32(0.575) * sigmoid32(logits) + f32(0.425) * ((rrf - lo) / rng).astype(f32)
    idx = sorted(range(len(logits)), key=lambda i: -blended[i])  # sorted() is stable
    return [(i, float(blended[i])) for i in idx]


def test_weights_are_the_reference_s():
    assert rerank.RERANK_WEIGHT == 0.575 and rerank.RRF_WEIGHT == 0.425  # neural.rs:12-13
    assert abs(rerank.RERANK_WEIGHT + rerank.RRF_WEIGHT - 1.0) < 1e-12


@pytest.mark.parametrize("n,seed", [(1, 0), (2, 1), (7, 2), (100, 3), (1000, 4)])
def test_blend_matches_the_reference_arithmetic(n, seed):
    rng = np.random.default_rng(seed)
    logits = rng.normal(0.0, 4.0, n).astype(f32)
    rrf = (rng.random(n) * 0.1).astype(f32)
    got = rerank.blend(logits, rrf)
    want = reference_blend(logits, rrf)
    assert sorted(i for i, _ in got) == list(range(n))
    by_index = dict(want)
    for i, s in got:
        assert abs(s - by_index[i]) <= 1e-6, (i, s, by_index[i])
    scores = [s for _, s in got]
    assert all(a >= b for a, b in zip(scores, scores[1:]))
    # the order is the reference's wherever its scores are further apart than the tolerance
    for (gi, gs), (wi, ws) in zip(got, want):
        assert gi == wi or abs(gs - ws) <= 2e-6


def test_order_is_stable_descending_with_nan_last():
    scores = np.array([0.5, 2.0, 0.5, np.nan, -1.0, 2.0, 0.5, np.nan, np.inf, -np.inf], f32)
    got = rerank.order(scores)
    assert [i for i, _ in got] == [8, 1, 5, 0, 2, 6, 4, 9, 3, 7]
    assert [s for _, s in got[:8]] == [float(scores[i]) for i in (8, 1, 5, 0, 2, 6, 4, 9)] and all(np.isnan(s) for _, s in got[8:])


def test_ties_keep_index_order_in_the_blend():
    logits = np.array([1.0, 1.0, -3.0, 1.0, -3.0], f32)
    rrf = np.array([0.02, 0.02, 0.01, 0.02, 0.01], f32)
    assert [i for i, _ in rerank.blend(logits, rrf)] == [0, 1, 3, 2, 4]


def test_constant_rrf_scores_meet_the_floor():
    """max - min = 0: the range is the 0.0001 floor (neural.rs:105), every normalised rrf is 0, and the blend is
    0.575 * sigmoid alone — no division by zero."""
    logits = np.array([-2.0, 0.0, 3.0], f32)
    got = dict(rerank.blend(logits, np.full(3, 0.0163, f32)))
    for i, x in enumerate(logits):
        assert abs(got[i] - float(f32(0.575) * sigmoid32(x))) <= 1e-6
    # a spread below the floor is divided by the floor, not by itself
    rrf = np.array([0.01, 0.01002, 0.01005], f32)
    got = dict(rerank.blend(np.zeros(3, f32), rrf))
    for i in range(3):
        want = f32(0.575) * f32(0.5) + f32(0.425) * (f32(rrf[i] - rrf[0]) / f32(0.0001))
        assert abs(got[i] - float(want)) <= 1e-6


def test_sigmoid():
    """neural.rs:133-138 (test_sigmoid), through the blend with constant rrf scores: blended / 0.575 = sigmoid."""
    got = dict(rerank.blend(np.array([0.0, 10.0, -10.0], f32), np.zeros(3, f32)))
    sig = {i: s / 0.575 for i, s in got.items()}
    assert abs(sig[0] - 0.5) < 0.0001
    assert sig[1] > 0.99
    assert sig[2] < 0.01


def test_empty_and_single():
    assert rerank.order(np.zeros(0, f32)) == [] and rerank.blend(np.zeros(0, f32), np.zeros(0, f32)) == []
    lib = _lib.load()
    assert lib.cs_rerank_order(None, 0, None, None) == _lib.CS_OK and lib.cs_rerank_blend(None, None, 0, None, None) == _lib.CS_OK
    assert rerank.order(np.array([-1.5], f32)) == [(0, -1.5)]
    (i, s), = rerank.blend(np.array([0.0], f32), np.array([0.3], f32))
    assert i == 0 and abs(s - 0.2875) <= 1e-6
    assert lib.cs_rerank_order(None, 3, None, None) == _lib.CS_ERR_BAD_ARG
    with pytest.raises(ValueError):
        rerank.blend(np.zeros(2, f32), np.zeros(3, f32))


# ---- the search step (src/search/mod.rs:712-722, :829-885) ----

def _result(i, score, path="src/a.rs"):
    return SearchResult(id=i, content=f"chunk {i}", path=path, start_line=1, end_line=2, kind="function", signature=None,
                        docstring=None, context=None, hash=str(i), distance=0.0, score=score)


class _FakeReranker:
    """rerank_and_blend through the host blend with logits = -(content's chunk number)"""

    def rerank_and_blend(self, query, documents, rrf_scores):
        return rerank.blend([-float(d.split()[1]) for d in documents], rrf_scores)


def test_search_step_takes_reranks_filters_and_truncates():
    assert rerank_take_count(50, 10, True, 30) == 30 and rerank_take_count(20, 10, True, 30) == 20
    assert rerank_take_count(50, 10, True) == 10 and rerank_take_count(50, 10, False) == 10
    assert rerank_take_count(50, 10, False, filter_by_path=True) == 30
    results = [_result(3, 0.030), _result(1, 0.020, "tests/b.rs"), _result(2, 0.010)]
    out = rerank_step(_FakeReranker(), "q", results, 2)
    want = rerank.blend([-3.0, -1.0, -2.0], [0.030, 0.020, 0.010])
    assert [r.id for r in out] == [results[i].id for i, _ in want[:2]]
    assert [r.score for r in out] == [s for _, s in want[:2]]
    assert [r.id for r in rerank_step(_FakeReranker(), "q", results, 5, filter_path="./src")] == [r.id for r in rerank_step(_FakeReranker(), "q", results, 5) if r.path.startswith("src")]
    assert [r.id for r in rerank_step(None, "q", results, 2)] == [3, 1]      # reranker off: as they came
    assert rerank_step(_FakeReranker(), "q", [], 5) == []


# ---- the head's loader ----

CFG = BertConfig(vocab_size=64, hidden=384, layers=1, heads=12, intermediate=1536, max_position=32, pooling=POOL_CLS)


def seeded_head(seed, H=384):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 0.05, (H, H)).astype(f32), rng.normal(0, 0.1, H).astype(f32), rng.normal(0, 0.05, (1, H)).astype(f32),
            rng.normal(0, 0.1, 1).astype(f32))


def write_checkpoint(path, scheme, head, prefix="bert.", dtype=np.float32, encoder=False, labels=1):
    from safetensors.numpy import save_file

    w_p, b_p, w_c, b_c = head
    if labels != 1:
        w_c, b_c = np.repeat(w_c, labels, 0), np.repeat(b_c, labels)
    if scheme == "bert":      # BertForSequenceClassification
        sd = {prefix + "pooler.dense.weight": w_p, prefix + "pooler.dense.bias": b_p, "classifier.weight": w_c, "classifier.bias": b_c}
    else:                     # RobertaForSequenceClassification
        sd = {"classifier.dense.weight": w_p, "classifier.dense.bias": b_p, "classifier.out_proj.weight": w_c,
              "classifier.out_proj.bias": b_c}
    if encoder:
        sd.update({prefix + k: v for k, v in to_state_dict(CFG, synth_params(CFG, 5)).items()})
    save_file({k: np.ascontiguousarray(v.astype(dtype)) for k, v in sd.items()}, str(path))


@pytest.mark.parametrize("scheme,prefix", [("bert", "bert."), ("bert", ""), ("roberta", "roberta.")])
def test_head_is_read_under_both_naming_schemes(tmp_path, scheme, prefix):
    head = seeded_head(11)
    p = tmp_path / "model.safetensors"
    write_checkpoint(p, scheme, head, prefix)
    got = rerank.head_from_safetensors(p, CFG)
    assert got.size == rerank.head_count(CFG) == 384 * 384 + 384 + 384 + 1
    assert np.array_equal(got, rerank.pack_head(*head))
    H = 384
    assert np.array_equal(got[:H * H].reshape(H, H), head[0]) and got[-1] == head[3][0]   # W_p | b_p | w_c | b_c, W_p row j = output j
    write_checkpoint(p, scheme, head, prefix, dtype=np.float16)
    assert np.array_equal(rerank.head_from_safetensors(p, CFG), rerank.pack_head(*[a.astype(np.float16) for a in head]))


def test_head_refusals_are_worded(tmp_path):
    from safetensors.numpy import save_file

    lib = _lib.load()
    p = tmp_path / "model.safetensors"
    head = seeded_head(12)

    def expect(code, needle, cfg=CFG):
        with pytest.raises(_lib.CsError) as e:
            rerank.head_from_safetensors(p, cfg)
        assert e.value.code == code and needle in str(e.value), (e.value.code, str(e.value))

    save_file({k: np.ascontiguousarray(v) for k, v in to_state_dict(CFG, synth_params(CFG, 5)).items() if "pooler" not in k}, str(p))
    expect(_lib.CS_ERR_BAD_ARG, "no score head")                         # an embedding model: no head at all
    write_checkpoint(p, "bert", head, labels=2)
    expect(_lib.CS_ERR_UNSUPPORTED, "num_labels 2")
    write_checkpoint(p, "roberta", head, labels=3)
    expect(_lib.CS_ERR_UNSUPPORTED, "num_labels 3")
    write_checkpoint(p, "bert", head)
    wide = BertConfig(vocab_size=64, hidden=768, layers=1, heads=12, intermediate=3072, max_position=32, pooling=POOL_CLS)
    expect(_lib.CS_ERR_DIM_MISMATCH, "pooler.dense.weight", wide)         # a 384-wide head for a 768-wide encoder
    out = np.empty(10, f32)
    ccfg = CFG.to_c()
    assert lib.cs_rerank_head_from_safetensors(str(p).encode(), C.byref(ccfg), out.ctypes.data_as(_lib.f32p), 10) == _lib.CS_ERR_BAD_ARG
    assert lib.cs_rerank_head_count(C.byref(ccfg)) == rerank.head_count(CFG)


def test_directory_refusals_come_before_the_device(tmp_path):
    """cs_reranker_create_from_dir refuses what it cannot run while it reads the directory, before it asks for a device."""
    lib = _lib.load()
    config = {"model_type": "bert", "architectures": ["BertForSequenceClassification"], "vocab_size": CFG.vocab_size, "hidden_size": 384,
              "num_hidden_layers": 1, "num_attention_heads": 12, "intermediate_size": 1536, "max_position_embeddings": 32,
              "type_vocab_size": 2, "layer_norm_eps": 1e-12, "hidden_act": "gelu"}

    def create(cfg_json):
        (tmp_path / "config.json").write_text(json.dumps(cfg_json))
        h = C.c_void_p()
        rc = lib.cs_reranker_create_from_dir(str(tmp_path).encode(), 0, C.byref(h))
        if rc == _lib.CS_OK:
            lib.cs_reranker_destroy(h)
        return rc, lib.cs_last_error().decode()

    write_checkpoint(tmp_path / "model.safetensors", "bert", seeded_head(13), encoder=True)
    rc, msg = create({**config, "num_labels": 2})
    assert rc == _lib.CS_ERR_UNSUPPORTED and "num_labels 2" in msg
    rc, msg = create({**config, "id2label": {"0": "a", "1": "b", "2": "c"}})
    assert rc == _lib.CS_ERR_UNSUPPORTED and "num_labels 3" in msg
    rc, msg = create({**config, "id2label": {"0": "LABEL_0"}})            # a good directory: only the device can be missing
    assert rc == _lib.CS_OK or (rc in (_lib.CS_ERR_HIP, _lib.CS_ERR_OOM) and lib.cs_device_count() <= 0), msg
    # no head in the checkpoint
    from safetensors.numpy import save_file

    save_file({"bert." + k: np.ascontiguousarray(v) for k, v in to_state_dict(CFG, synth_params(CFG, 5)).items() if "pooler" not in k},
              str(tmp_path / "model.safetensors"))
    rc, msg = create(config)
    assert rc == _lib.CS_ERR_BAD_ARG and "no score head" in msg
    # an ONNX export / a quantised export instead of the checkpoint
    (tmp_path / "model.safetensors").unlink()
    (tmp_path / "onnx").mkdir()
    (tmp_path / "onnx" / "model_quantized.onnx").write_bytes(b"")
    rc, msg = create(config)
    assert rc == _lib.CS_ERR_UNSUPPORTED and "quantised" in msg
    (tmp_path / "onnx" / "model_quantized.onnx").rename(tmp_path / "onnx" / "model.onnx")
    rc, msg = create(config)
    assert rc == _lib.CS_ERR_UNSUPPORTED and "ONNX" in msg
    # ModernBERT has no token types and is not built as a cross-encoder
    ccfg = BertConfig(vocab_size=64, hidden=768, layers=1, heads=12, intermediate=1152, max_position=32, pooling=POOL_CLS, arch=4,
                      rotary_base=160000.0, rotary_base_local=10000.0, local_window=64, global_every=3).to_c()
    head = np.zeros(768 * 768 + 2 * 768 + 1, f32)
    h = C.c_void_p()
    rc = lib.cs_reranker_create(C.byref(ccfg), None, head.ctypes.data_as(_lib.f32p), 1, 0, C.byref(h))
    assert rc == _lib.CS_ERR_UNSUPPORTED and "ModernBERT" in lib.cs_last_error().decode()
