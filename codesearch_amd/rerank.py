"""Host-side mirror of the reference's NeuralReranker (src/rerank/neural.rs): a cross-encoder scores every (query, chunk
content) pair, `rerank` orders by that score, `rerank_and_blend` blends its sigmoid with the min-max-normalised fusion
score.  The scoring runs on the device behind cs_reranker_* of the C ABI (csrc/reranker.hip, csrc/rerank_head.hip); the
ordering and the blend are csrc/rerank_host.cpp.  There is no CPU fallback.

fastembed's TextRerank (JINARerankerV1TurboEn by default) is restated from memory in three places that no source this
project holds pins down: it truncates at 512 tokens, returns raw logits and sorts by score, descending."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import f32p, i32p, u32p
from .bert_params import BertConfig
from .tokenizer import pack_texts

RERANK_WEIGHT = 0.575  # neural.rs:12
RRF_WEIGHT = 0.425     # neural.rs:13
DEFAULT_MAX_LENGTH = 512


def head_count(cfg: BertConfig) -> int:
    """Floats of a score head: W_p [H, H] | b_p [H] | w_c [H] | b_c [1]."""
    return cfg.hidden * cfg.hidden + 2 * cfg.hidden + 1


def pack_head(w_p: np.ndarray, b_p: np.ndarray, w_c: np.ndarray, b_c) -> np.ndarray:
    """-> the flat head block of cs_reranker_create (w_p row j = output j, as torch's Linear.weight)."""
    return np.concatenate([np.asarray(w_p, np.float32).ravel(), np.asarray(b_p, np.float32).ravel(),
                           np.asarray(w_c, np.float32).ravel(), np.asarray(b_c, np.float32).ravel()])


def order(scores) -> List[Tuple[int, float]]:
    """cs_rerank_order: (index, score) by score descending, index ascending on ties, NaN last."""
    scores = np.ascontiguousarray(scores, np.float32)
    n = scores.size
    idx, out = np.empty(n, np.uint32), np.empty(n, np.float32)
    _lib.check(_lib.load().cs_rerank_order(scores.ctypes.data_as(f32p), n, idx.ctypes.data_as(u32p), out.ctypes.data_as(f32p)))
    return list(zip(idx.tolist(), out.tolist()))


def blend(logits, rrf_scores) -> List[Tuple[int, float]]:
    """cs_rerank_blend: neural.rs:96-118 on raw logits and fusion scores."""
    logits = np.ascontiguousarray(logits, np.float32)
    rrf = np.ascontiguousarray(rrf_scores, np.float32)
    if logits.size != rrf.size:
        raise ValueError("Documents and RRF scores must have same length")  # neural.rs:87-91
    n = logits.size
    idx, out = np.empty(n, np.uint32), np.empty(n, np.float32)
    _lib.check(_lib.load().cs_rerank_blend(logits.ctypes.data_as(f32p), rrf.ctypes.data_as(f32p), n, idx.ctypes.data_as(u32p),
                                           out.ctypes.data_as(f32p)))
    return list(zip(idx.tolist(), out.tolist()))


def head_from_safetensors(path: str, cfg: BertConfig) -> np.ndarray:
    """The score head of a sequence-classification checkpoint (cs_rerank_head_from_safetensors), flat."""
    head = np.empty(head_count(cfg), np.float32)
    ccfg = cfg.to_c()
    _lib.check(_lib.load().cs_rerank_head_from_safetensors(str(path).encode(), C.byref(ccfg), head.ctypes.data_as(f32p), head.size))
    return head


class NeuralReranker:
    """neural.rs:17-122.  `head` = the flat block of pack_head; `params` as FastEmbedder's (None: synthetic encoder weights
    from `seed`).  `tokenizer`: a WordPieceTokenizer whose handle has a pair form (tokenizer.encode_pairs)."""

    def __init__(self, config: BertConfig, head: np.ndarray, params: Optional[np.ndarray] = None, seed: int = 0, device: int = 0,
                 tokenizer=None, max_length: int = DEFAULT_MAX_LENGTH, model_name: str = "jina-reranker-v1-turbo-en"):
        self._lib = _lib.load()
        self.config = config
        self.tokenizer = tokenizer
        self.max_length = max_length
        self._model_name = model_name
        ccfg = config.to_c()
        head = np.ascontiguousarray(head, np.float32)
        if head.size != head_count(config):
            raise _lib.CsError(_lib.CS_ERR_DIM_MISMATCH, f"Failed to initialize reranker model: expected {head_count(config)} head "
                                                         f"parameters, got {head.size}")
        pptr = None
        if params is not None:
            params = np.ascontiguousarray(params, np.float32)
            need = int(self._lib.cs_bert_param_count(C.byref(ccfg)))
            if params.size != need:
                raise _lib.CsError(_lib.CS_ERR_DIM_MISMATCH, f"Failed to initialize reranker model: expected {need} parameters, got {params.size}")
            pptr = params.ctypes.data_as(f32p)
        h = C.c_void_p()
        _lib.check(self._lib.cs_reranker_create(C.byref(ccfg), pptr, head.ctypes.data_as(f32p), seed, device, C.byref(h)))
        self._h = h

    @classmethod
    def from_dir(cls, model_dir: str, device: int = 0, max_length: int = DEFAULT_MAX_LENGTH) -> "NeuralReranker":
        """A sequence-classification snapshot: config.json, model.safetensors, tokenizer.json or vocab.txt
        (cs_reranker_create_from_dir + cs_tokenizer_create_from_dir)."""
        from .tokenizer import WordPieceTokenizer

        self = cls.__new__(cls)
        self._lib = _lib.load()
        ccfg = _lib.BertConfig()
        _lib.check(self._lib.cs_bert_config_from_dir(str(model_dir).encode(), 0, C.byref(ccfg)))
        self.config = BertConfig(vocab_size=ccfg.vocab_size, hidden=ccfg.hidden, layers=ccfg.layers, heads=ccfg.heads,
                                 intermediate=ccfg.intermediate, max_position=ccfg.max_position,
                                 type_vocab_size=ccfg.type_vocab_size, layer_norm_eps=ccfg.layer_norm_eps,
                                 pooling=ccfg.pooling, arch=ccfg.arch, rotary_base=ccfg.rotary_base,
                                 rotary_base_local=ccfg.rotary_base_local, local_window=ccfg.local_window,
                                 global_every=ccfg.global_every)
        h = C.c_void_p()
        _lib.check(self._lib.cs_reranker_create_from_dir(str(model_dir).encode(), device, C.byref(h)))
        self._h = h
        self.max_length = max_length
        self._model_name = str(model_dir)
        self.tokenizer = WordPieceTokenizer.from_dir(str(model_dir), max_length=min(max_length, self.config.max_position))
        return self

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cs_reranker_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def model_name(self) -> str:
        return self._model_name

    @property
    def embedder_handle(self) -> C.c_void_p:
        """The encoder inside (borrowed): cs_embedder_last_hidden, the counters and the profiles of the scoring calls."""
        return C.c_void_p(self._lib.cs_reranker_embedder(self._h))

    def last_hidden(self, n_tokens: int) -> np.ndarray:
        out = np.empty((n_tokens, self.config.hidden), np.float32)
        _lib.check(self._lib.cs_embedder_last_hidden(self.embedder_handle, out.ctypes.data_as(f32p), n_tokens))
        return out

    def debug_counters(self):
        """-> (split_forwards, f32_forwards, range_fallbacks) of the encoder inside"""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _lib.check(self._lib.cs_embedder_debug_counters(self.embedder_handle, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def score_ids(self, ids, mask, types=None, batch_size: int = 0) -> np.ndarray:
        """ids / mask / types [n, L] int32 (types None: every token has type 0) -> [n] float32 raw logits."""
        ids = np.ascontiguousarray(ids, np.int32)
        mask = np.ascontiguousarray(mask, np.int32)
        if ids.ndim != 2 or ids.shape != mask.shape:
            raise ValueError("ids and mask must both be [n, seq_len]")
        tptr = None
        if types is not None:
            types = np.ascontiguousarray(types, np.int32)
            if types.shape != ids.shape:
                raise ValueError("types must be [n, seq_len] like ids")
            tptr = types.ctypes.data_as(i32p)
        n, L = ids.shape
        out = np.empty(n, np.float32)
        _lib.check(self._lib.cs_reranker_score_ids(self._h, ids.ctypes.data_as(i32p), mask.ctypes.data_as(i32p), tptr, n, L,
                                                   batch_size, out.ctypes.data_as(f32p), None))
        return out

    def _rerank_texts(self, query: str, documents: Sequence[str], rrf_scores) -> List[Tuple[int, float]]:
        if self.tokenizer is None:
            raise _lib.CsError(_lib.CS_ERR_BAD_ARG, "Failed to rerank: no tokenizer attached")
        n = len(documents)
        blob, offsets = pack_texts(documents)
        idx, out = np.empty(n, np.uint32), np.empty(n, np.float32)
        rptr = None
        if rrf_scores is not None:
            rrf_scores = np.ascontiguousarray(rrf_scores, np.float32)
            rptr = rrf_scores.ctypes.data_as(f32p)
        _lib.check(self._lib.cs_reranker_rerank_texts(self._h, self.tokenizer.handle, query.encode("utf-8", "replace"), blob,
                                                      offsets.ctypes.data_as(_lib.u64p), n, self.max_length, rptr,
                                                      idx.ctypes.data_as(u32p), out.ctypes.data_as(f32p)))
        return list(zip(idx.tolist(), out.tolist()))

    def rerank(self, query: str, documents: Sequence[str]) -> List[Tuple[int, float]]:
        """neural.rs:56-72: (original index, rerank score), score descending."""
        if not documents:
            return []
        return self._rerank_texts(query, documents, None)

    def rerank_and_blend(self, query: str, documents: Sequence[str], rrf_scores: Sequence[float]) -> List[Tuple[int, float]]:
        """neural.rs:77-121: (original index, RERANK_WEIGHT * sigmoid(score) + RRF_WEIGHT * min-max(rrf)), descending."""
        if not documents:
            return []
        if len(documents) != len(rrf_scores):
            raise ValueError("Documents and RRF scores must have same length")  # neural.rs:87-91
        return self._rerank_texts(query, documents, rrf_scores)
