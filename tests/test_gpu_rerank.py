"""Cross-encoder reranking on the device (cs_reranker_*: csrc/reranker.hip, the score head of csrc/rerank_head.hip, the
token types of the embedding kernels) against float64 references: the head alone on the GPU's own CLS rows, the whole
model against the oracle's encoder + a float64 head on every dense-layer route, token types through an equivalent
vocabulary, an independent golden written by HF BertForSequenceClassification (tests/golden/make_rerank_golden.py), the text
entry points on snapshots written here, batch invariance, repeatability and the refusals.

Shapes: hidden 384, 12 heads, intermediate 1536, vocabulary 512, two layers.  The head is drawn N(0, 0.05) with biases
N(0, 0.1): a transposed W_p, a missing tanh or a dropped bias then moves a logit by about the logits' whole spread."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from codesearch_amd import _lib, rerank
from codesearch_amd.bert_params import (ARCH_BERT, ARCH_JINA, ARCH_MODERN, POOL_CLS, BertConfig, synth_params, synth_token_batch,
                                        to_state_dict)
from codesearch_amd.rerank import NeuralReranker

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
H = 384
TOL_CLS = 2e-4          # the project's bound on a hidden state against the oracle (tests/test_gpu_encoder.py, test_gpu_jina.py)
ARCHS = {"bert": ARCH_BERT, "jina": ARCH_JINA}
PARAM_SEED, HEAD_SEED = 1234, 77


def config(arch, hidden=H, heads=12, intermediate=1536, layers=2):
    return BertConfig(vocab_size=512, hidden=hidden, layers=layers, heads=heads, intermediate=intermediate, max_position=512,
                      pooling=POOL_CLS, arch=arch)


def seeded_head(seed, hidden=H):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 0.05, (hidden, hidden)).astype(np.float32), rng.normal(0, 0.1, hidden).astype(np.float32),
            rng.normal(0, 0.05, hidden).astype(np.float32), rng.normal(0, 0.1, 1).astype(np.float32))


def head_f64(head, x):
    """float64 head on rows x [n, H] -> (logits [n], forward error bound of the f32 kernel [n]).
    gamma = (H + 2) 2^-23 covers a dot product of H terms plus the bias in any order; 2.4e-7 is tanhf's error."""
    w_p, b_p, w_c, b_c = (a.astype(np.float64) for a in head)
    x = x.astype(np.float64)
    gamma = (x.shape[1] + 2) * 2.0 ** -23
    z = x @ w_p.T + b_p
    bound_z = gamma * (np.abs(x) @ np.abs(w_p).T + np.abs(b_p))
    t = np.tanh(z)
    logits = t @ w_c + b_c[0]
    bound = (bound_z + 2.4e-7) @ np.abs(w_c) + gamma * (np.abs(t) @ np.abs(w_c) + abs(b_c[0]))
    return logits, bound


def l1_bound(head):
    """sum_j |w_cj| sum_k |W_jk|: how far a logit moves per unit of max-norm distance between two CLS rows (tanh is 1-Lipschitz)"""
    w_p, _, w_c, _ = (a.astype(np.float64) for a in head)
    return float(np.abs(w_c) @ np.abs(w_p).sum(1))


_PARAMS = {}


def params_of(arch):
    if arch not in _PARAMS:
        _PARAMS[arch] = synth_params(config(ARCHS[arch]), PARAM_SEED)
    return _PARAMS[arch]


@pytest.fixture(scope="module", params=list(ARCHS))
def model(request):
    arch = request.param
    head = seeded_head(HEAD_SEED)
    rr = NeuralReranker(config(ARCHS[arch]), rerank.pack_head(*head), params=params_of(arch))
    yield arch, rr, head
    rr.close()


_ORACLE = {}


def oracle_cls(oracle, arch, params, ids, mask, key):
    """The oracle's CLS rows of the last layer, computed once per case and shared."""
    if key not in _ORACLE:
        _ORACLE[key] = oracle.bert_forward(config(ARCHS[arch]), params, ids, mask, want_hidden=True)["hidden"][:, 0, :].copy()
    return _ORACLE[key]


def no_f32_fallback(rr, before):
    split, f32, fallbacks = rr.debug_counters()
    assert f32 == before[1] and fallbacks == before[2] and split > before[0], (before, (split, f32, fallbacks))


# ---- the head alone ----

def test_head_alone_on_the_gpus_own_cls_rows(model):
    arch, rr, head = model
    B, L = 37, 24          # 888 tokens (under the CLS tail's 4,096), five head blocks, the last one partly filled
    ids, mask = synth_token_batch(rr.config, 5, B, L, True)
    logits = rr.score_ids(ids, mask)
    cls = rr.last_hidden(B * L).reshape(B, L, H)[:, 0, :]
    want, bound = head_f64(head, cls)
    print("head alone", arch, "max |diff|", np.abs(logits - want).max(), "bound", bound.min(), "logit spread", want.std())
    assert (np.abs(logits - want) <= bound).all(), (np.abs(logits - want).max(), bound.min())
    # the check has something to see: the same head with W_p transposed, or without its tanh, lands outside the bound
    transposed, _ = head_f64((head[0].T.copy(),) + head[1:], cls)
    linear = (cls.astype(np.float64) @ head[0].astype(np.float64).T + head[1]) @ head[2].astype(np.float64) + float(head[3][0])
    assert (np.abs(transposed - want) > bound).mean() > 0.9 and (np.abs(linear - want) > bound).mean() > 0.9


@pytest.mark.parametrize("hidden,heads,intermediate", [(768, 12, 3072), (1024, 16, 4096)])
def test_head_alone_at_the_other_widths(hidden, heads, intermediate):
    cfg = config(ARCH_BERT, hidden, heads, intermediate, layers=1)
    head = seeded_head(HEAD_SEED + hidden, hidden)
    rr = NeuralReranker(cfg, rerank.pack_head(*head), seed=9)
    B, L = 11, 16
    ids, mask = synth_token_batch(cfg, 6, B, L, True)
    logits = rr.score_ids(ids, mask)
    cls = rr.last_hidden(B * L).reshape(B, L, hidden)[:, 0, :]
    want, bound = head_f64(head, cls)
    assert (np.abs(logits - want) <= bound).all(), (np.abs(logits - want).max(), bound.min())
    rr.close()


# ---- end to end against the oracle: one shape per dense-layer route ----

SHAPES = [(5, 24), (9, 40), (40, 64), (64, 256)]   # small path | skinny kernels | mid-size tiles | wide kernels (BERT: + the CLS tail)


@pytest.mark.parametrize("B,L", SHAPES)
def test_end_to_end_against_the_oracle(model, oracle, B, L):
    arch, rr, head = model
    ids, mask = synth_token_batch(rr.config, 100 + B, B, L, True)
    assert mask.sum() < B * L                                   # ragged
    ref_cls = oracle_cls(oracle, arch, params_of(arch), ids, mask, (arch, B, L))
    before = rr.debug_counters()
    logits = rr.score_ids(ids, mask)
    no_f32_fallback(rr, before)
    if arch == "bert" and B * L >= 4096:
        # the CLS tail ran (the head read its compact rows): the last layer exists for the CLS rows only
        with pytest.raises(_lib.CsError) as e:
            rr.last_hidden(B * L)
        assert e.value.code == _lib.CS_ERR_UNSUPPORTED
        # the CLS rows through the encoder's own output stage: L2-normalised, so the bound is divided by the smallest norm
        out = np.empty((B, H), np.float32)
        _lib.check(_lib.load().cs_embedder_embed_ids(rr.embedder_handle, ids.ctypes.data_as(_lib.i32p), mask.ctypes.data_as(_lib.i32p),
                                                     B, L, 0, out.ctypes.data_as(_lib.f32p), None))
        norms = np.linalg.norm(ref_cls.astype(np.float64), axis=1, keepdims=True)
        np.testing.assert_allclose(out, ref_cls / norms, atol=TOL_CLS / norms.min())
    else:
        cls = rr.last_hidden(B * L).reshape(B, L, H)[:, 0, :]
        np.testing.assert_allclose(cls, ref_cls, atol=TOL_CLS)
    want, bound = head_f64(head, ref_cls)
    tol = l1_bound(head) * TOL_CLS + bound
    print("end to end", arch, (B, L), "max |diff|", np.abs(logits - want).max(), "tolerance", tol.min())
    assert (np.abs(logits - want) <= tol).all(), (np.abs(logits - want).max(), tol.min())


# ---- token types ----

def typed_params(arch):
    """Type row 0 all zero and word row a + 256 = fl32(word[a] + type[1]): ids a with type 1 are then the same model input,
    bit for bit, as ids a + 256 with type 0."""
    flat = params_of(arch).copy()
    sd = to_state_dict(config(ARCHS[arch]), flat)   # views into flat
    word, typ = sd["embeddings.word_embeddings.weight"], sd["embeddings.token_type_embeddings.weight"]
    typ[0] = 0.0
    word[256:512] = word[0:256] + typ[1]
    return flat


@pytest.fixture(scope="module", params=list(ARCHS))
def typed_model(request):
    arch = request.param
    head = seeded_head(HEAD_SEED + 1)
    flat = typed_params(arch)
    rr = NeuralReranker(config(ARCHS[arch]), rerank.pack_head(*head), params=flat)
    yield arch, rr, head, flat
    rr.close()


@pytest.mark.parametrize("B,L", [(5, 24), (30, 40)])   # the small path | 1,200 token rows: the embedding kernel of every other route
def test_token_types_select_the_type_row(typed_model, oracle, B, L):
    arch, rr, head, flat = typed_model
    rng = np.random.default_rng(B)
    lens = rng.integers(max(2, L // 4), L + 1, B)
    lens[0] = L
    mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int32)
    ids = (rng.integers(1, 256, (B, L)) * mask).astype(np.int32)
    # a pair's layout: type 0 up to a row's own border, type 1 behind it, 0 on the padding
    border = rng.integers(1, lens)
    types = ((np.arange(L)[None, :] >= border[:, None]) & (mask == 1)).astype(np.int32)
    assert types.any() and (types == 0).any()
    untyped = rr.score_ids(ids, mask, None)
    typed = rr.score_ids(ids, mask, types)
    moved = rr.score_ids(ids + 256 * types, mask, np.zeros_like(types))
    assert np.array_equal(typed.view(np.uint32), moved.view(np.uint32))
    assert np.array_equal(rr.score_ids(ids + 256 * types, mask, None).view(np.uint32), moved.view(np.uint32))   # NULL = all zero
    assert np.abs(typed - untyped).max() > 1e-3                                      # the types are not ignored
    ref_cls = oracle_cls(oracle, arch, flat, ids + 256 * types, mask, ("typed", arch, B, L))
    cls = rr.last_hidden(B * L).reshape(B, L, H)[:, 0, :]
    np.testing.assert_allclose(cls, ref_cls, atol=TOL_CLS)
    want, bound = head_f64(head, ref_cls)
    assert (np.abs(moved - want) <= l1_bound(head) * TOL_CLS + bound).all()


# ---- an independent golden: HF BertForSequenceClassification in float64 ----

def test_golden_of_hf_bert_for_sequence_classification():
    g = np.load(os.path.join(HERE, "golden", "rerank_golden.npz"))
    cfg = BertConfig(vocab_size=int(g["vocab_size"]), hidden=H, layers=int(g["layers"]), heads=12, intermediate=1536,
                     max_position=int(g["max_position"]), pooling=POOL_CLS)
    head = seeded_head(int(g["head_seed"]))
    rr = NeuralReranker(cfg, rerank.pack_head(*head), params=synth_params(cfg, int(g["param_seed"])))
    ids, mask, types = g["ids"], g["mask"], g["types"]
    assert types.any()
    logits = rr.score_ids(ids, mask, types)
    B, L = ids.shape
    _, bound = head_f64(head, rr.last_hidden(B * L).reshape(B, L, H)[:, 0, :])
    tol = l1_bound(head) * TOL_CLS + bound
    print("golden max |diff|", np.abs(logits - g["logits"]).max(), "tolerance", tol.min())
    assert (np.abs(logits - g["logits"]) <= tol).all(), (logits, g["logits"])
    rr.close()


# ---- texts ----

QUERY = "How do I authenticate users?"
DOCUMENTS = ["fn authenticate(user: &str, password: &str) -> bool { ... }", "fn calculate_sum(a: i32, b: i32) -> i32 { a + b }",
             "impl UserAuth for App { fn login(&self, credentials: Credentials) -> Result<Token> }"]   # neural.rs:163-169


def bert_snapshot(d):
    """A BertForSequenceClassification snapshot: bert.* encoder names, bert.pooler.dense + classifier, vocab.txt."""
    from safetensors.numpy import save_file

    from codesearch_amd.pipeline import synth_vocab

    vocab = synth_vocab(448)
    for w in "how do i authenticate users fn user password bool sum impl for app login self result token a b".split():
        vocab.setdefault(w, len(vocab))
    cfg = BertConfig(vocab_size=len(vocab), hidden=H, layers=2, heads=12, intermediate=1536, max_position=64, pooling=POOL_CLS)
    flat, head = synth_params(cfg, 31), seeded_head(32)
    sd = {"bert." + k: np.ascontiguousarray(v) for k, v in to_state_dict(cfg, flat).items()}
    sd.update({"bert.pooler.dense.weight": head[0], "bert.pooler.dense.bias": head[1], "classifier.weight": head[2][None, :],
               "classifier.bias": head[3]})
    os.makedirs(d)
    save_file(sd, os.path.join(d, "model.safetensors"))
    json.dump({"model_type": "bert", "architectures": ["BertForSequenceClassification"], "vocab_size": cfg.vocab_size, "hidden_size": H,
               "num_hidden_layers": 2, "num_attention_heads": 12, "intermediate_size": 1536, "max_position_embeddings": 64,
               "type_vocab_size": 2, "layer_norm_eps": 1e-12, "hidden_act": "gelu", "id2label": {"0": "LABEL_0"}},
              open(os.path.join(d, "config.json"), "w"))
    open(os.path.join(d, "vocab.txt"), "w", encoding="utf-8").write("\n".join(sorted(vocab, key=vocab.get)) + "\n")
    json.dump({"do_lower_case": True, "model_max_length": 64}, open(os.path.join(d, "tokenizer_config.json"), "w"))
    from tokenizers import Tokenizer, models, normalizers, pre_tokenizers, processors

    tk = Tokenizer(models.WordPiece(vocab, unk_token="[UNK]", max_input_chars_per_word=100))
    tk.normalizer = normalizers.BertNormalizer(lowercase=True)
    tk.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    tk.post_processor = processors.BertProcessing(sep=("[SEP]", vocab["[SEP]"]), cls=("[CLS]", vocab["[CLS]"]))
    return tk, vocab["[PAD]"]


def jina_cross_encoder_snapshot(d):
    """A JinaBert sequence-classification snapshot (the reference's default reranker's family) with a byte-level BPE
    tokenizer.json under RobertaProcessing."""
    from safetensors.numpy import load_file, save_file

    from tests.test_bpe_tokenizer import build as build_bpe
    from tests.test_gpu_jina import jina_snapshot

    cfg = BertConfig(vocab_size=704, hidden=H, layers=2, heads=12, intermediate=1536, max_position=512, pooling=POOL_CLS, arch=ARCH_JINA)
    flat, head = synth_params(cfg, 41), seeded_head(42)
    sd = to_state_dict(cfg, flat)
    for l in range(cfg.layers):     # the family's gated projection has no bias
        sd[f"encoder.layer.{l}.intermediate.dense.bias"][:] = 0
        sd[f"encoder.layer.{l}.intermediate.gate.bias"][:] = 0
    jina_snapshot(d, cfg, flat)
    st = {"bert." + k: v for k, v in load_file(os.path.join(d, "model.safetensors")).items()}
    st.update({"bert.pooler.dense.weight": head[0], "bert.pooler.dense.bias": head[1], "classifier.weight": head[2][None, :],
               "classifier.bias": head[3]})
    save_file(st, os.path.join(d, "model.safetensors"))
    hf = json.load(open(os.path.join(d, "config.json")))
    hf["num_labels"] = 1
    json.dump(hf, open(os.path.join(d, "config.json"), "w"))
    tk = build_bpe(os.path.join(d, "tokenizer.json"), post="roberta")
    assert tk.get_vocab_size() <= cfg.vocab_size
    return tk, tk.token_to_id("<pad>")


@pytest.mark.parametrize("family", ["bert_wordpiece", "jina_bpe"])
def test_texts_from_a_snapshot(tmp_path, family):
    pytest.importorskip("tokenizers")
    d = str(tmp_path / "snapshot")
    tk, pad = bert_snapshot(d) if family == "bert_wordpiece" else jina_cross_encoder_snapshot(d)
    rr = NeuralReranker.from_dir(d, max_length=64)
    assert rr.config.arch == (ARCH_BERT if family == "bert_wordpiece" else ARCH_JINA) and rr.config.pooling == POOL_CLS
    docs = DOCUMENTS + ["", "x", "let total = values.iter().map(|v| v * 2).sum::<i64>(); " * 6]
    # neural.rs:160-180 (test_rerank_basic): every document once, scores descending
    results = rr.rerank(QUERY, DOCUMENTS)
    assert len(results) == 3 and sorted(i for i, _ in results) == [0, 1, 2]
    assert all(results[i][1] >= results[i + 1][1] for i in range(len(results) - 1))
    results = rr.rerank(QUERY, docs)
    assert sorted(i for i, _ in results) == list(range(len(docs)))
    assert all(a[1] >= b[1] for a, b in zip(results, results[1:]))
    # ... and they are score_ids on the library's own pair encodings, ordered by the host
    tk.enable_truncation(max_length=64)
    tk.enable_padding(pad_id=pad, pad_type_id=0, pad_token=tk.id_to_token(pad))
    enc = tk.encode_batch([(QUERY, t) for t in docs])
    ids = np.array([e.ids for e in enc], np.int32)
    mask = np.array([e.attention_mask for e in enc], np.int32)
    types = np.array([e.type_ids for e in enc], np.int32)
    assert ids.shape[1] == 64 and (family == "jina_bpe" or types.any())
    mine = rr.tokenizer.encode_pairs(QUERY, docs, max_length=64)
    assert all(np.array_equal(a, b) for a, b in zip(mine, (ids, mask, types)))
    logits = rr.score_ids(ids, mask, types)
    want = rerank.order(logits)
    assert [i for i, _ in results] == [i for i, _ in want]
    # (rerank_texts pads each length group to its own longest pair: the same logits up to the batch-invariance bound)
    l1 = l1_bound(seeded_head(32 if family == "bert_wordpiece" else 42))
    assert max(abs(a[1] - b[1]) for a, b in zip(results, want)) <= 2e-6 * l1
    rrf = np.linspace(0.03, 0.01, len(docs)).astype(np.float32)
    blended = rr.rerank_and_blend(QUERY, docs, rrf)
    want = dict(rerank.blend(logits, rrf))      # the host blend of score_ids on the library's encodings
    assert sorted(i for i, _ in blended) == list(range(len(docs)))
    # (a logit may differ by the batch-invariance bound; the blend scales it by 0.575 * sigmoid' <= 0.575 / 4)
    assert all(abs(s - want[i]) <= 1e-6 + 0.575 / 4 * 2e-6 * l1 for i, s in blended)
    assert all(a[1] >= b[1] for a, b in zip(blended, blended[1:]))
    assert rr.rerank(QUERY, []) == [] and rr.rerank_and_blend(QUERY, [], []) == []     # neural.rs:57-59, :83-85
    rr.close()


# ---- invariance and repeatability ----

def test_a_pair_scores_the_same_alone_padded_and_behind_others(model):
    arch, rr, head = model
    L = 40
    ids, mask = synth_token_batch(rr.config, 8, 12, L, True)
    row = 3
    n = int(mask[row].sum())
    assert 2 <= n < L
    alone = rr.score_ids(ids[row:row + 1, :n], mask[row:row + 1, :n])[0]
    padded = rr.score_ids(ids[row:row + 1], mask[row:row + 1])[0]
    batch = rr.score_ids(ids, mask)
    behind = rr.score_ids(np.roll(ids, 5, 0), np.roll(mask, 5, 0))[(row + 5) % 12]
    tol = 2e-6 * l1_bound(head)
    print("invariance", arch, [abs(float(v) - float(alone)) for v in (padded, batch[row], behind)], "tolerance", tol)
    for v in (padded, batch[row], behind):
        assert abs(float(v) - float(alone)) <= tol
    again = rr.score_ids(ids, mask)
    assert np.array_equal(batch.view(np.uint32), again.view(np.uint32))          # identical calls, identical bits
    # more rows than one mini-batch: length-grouped windows scatter one float per row back into input order
    many_ids, many_mask = synth_token_batch(rr.config, 9, 70, L, True)
    whole = rr.score_ids(many_ids, many_mask, batch_size=16)
    one = rr.score_ids(many_ids, many_mask, batch_size=128)
    assert np.abs(whole - one).max() <= tol


# ---- refusals ----

def test_refusals(model, tmp_path):
    arch, rr, head = model
    lib = _lib.load()
    ids, mask = synth_token_batch(rr.config, 8, 4, 16, True)
    for bad in (2, -1):
        types = np.zeros_like(ids)
        types[1, 3] = bad
        with pytest.raises(_lib.CsError) as e:
            rr.score_ids(ids, mask, types)
        assert e.value.code == _lib.CS_ERR_BAD_ARG and "token type" in str(e.value)
    assert np.isfinite(rr.score_ids(ids, mask)).all()          # the handle is still good
    # a quantised mode cannot reach a reranker: its encoder is never a quantised model
    assert lib.cs_embedder_set_gemm_mode(rr.embedder_handle, _lib.CS_GEMM_Q8_DYNAMIC) == _lib.CS_ERR_UNSUPPORTED
    assert np.isfinite(rr.score_ids(ids, mask)).all()
    # blocks of another size: the C ABI takes them without a length (as cs_embedder_create takes params), so it is the
    # mirror that refuses them, before any call
    with pytest.raises(_lib.CsError) as e:                     # a head of another width
        NeuralReranker(rr.config, np.zeros(768 * 768 + 2 * 768 + 1, np.float32), seed=1)
    assert e.value.code == _lib.CS_ERR_DIM_MISMATCH
    with pytest.raises(_lib.CsError) as e:
        NeuralReranker(rr.config, rerank.pack_head(*head), params=np.zeros(10, np.float32))
    assert e.value.code == _lib.CS_ERR_DIM_MISMATCH
    modern = BertConfig(vocab_size=512, hidden=768, layers=1, heads=12, intermediate=1152, max_position=64, pooling=POOL_CLS, arch=ARCH_MODERN,
                        rotary_base=160000.0, rotary_base_local=10000.0, local_window=64, global_every=3)
    with pytest.raises(_lib.CsError) as e:
        NeuralReranker(modern, np.zeros(rerank.head_count(modern), np.float32), seed=1)
    assert e.value.code == _lib.CS_ERR_UNSUPPORTED and "ModernBERT" in str(e.value)
    # a quantised export in place of the checkpoint
    d = tmp_path / "q"
    (d / "onnx").mkdir(parents=True)
    (d / "onnx" / "model_quantized.onnx").write_bytes(b"")
    (d / "config.json").write_text(json.dumps({"model_type": "bert", "vocab_size": 512, "hidden_size": H, "num_hidden_layers": 1,
                                               "num_attention_heads": 12, "intermediate_size": 1536, "max_position_embeddings": 64,
                                               "type_vocab_size": 2, "layer_norm_eps": 1e-12, "hidden_act": "gelu"}))
    h = C.c_void_p()
    assert lib.cs_reranker_create_from_dir(str(d).encode(), 0, C.byref(h)) == _lib.CS_ERR_UNSUPPORTED
    assert "quantised" in lib.cs_last_error().decode()
