"""``MpnetEncoder``: the sentence encoder on the MI355X (MPNet, or BERT checkpoints such as all-MiniLM-L6-v2 and
bge-*-en-v1.5; ``parse_model_config``) behind the six
``SentenceTransformer`` members the reference touches:
``.to(dev)``, ``.max_seq_length``, ``.get_sentence_embedding_dimension()``,
``.device`` and ``.encode(str|list, batch_size=, normalize_embeddings=,
show_progress_bar=, convert_to_numpy=)`` (``src/embeddings.py:86-117``,
``:184-188``, ``:216-222``).

``encode`` semantics restated from sentence-transformers [from knowledge,
SURVEY.md App. A item 7]: a str gives a 1-D vector, a list gives ``[n, 768]``;
sentences are sorted by length (descending), processed in batches of
``batch_size``, truncated to ``max_seq_length`` tokens, and returned in input
order as float32.  Pooling(mean) + Normalize() are part of the model, so outputs
are unit norm even before ``normalize_embeddings=True`` re-normalises them.
Batches are packed var-len (no padding) before they cross the C ABI.
"""
from __future__ import annotations

import ctypes
import json
import logging
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from . import _native as nat
from .tokenizer import HashTokenizer, WordPieceTokenizer, make_wordpiece  # noqa: F401

DEFAULT_CFG = dict(num_layers=12, hidden=768, heads=12, ffn=3072, vocab=30527, max_pos=514, rel_buckets=32,
                   pad_id=1, max_seq_len=384, ln_eps=1e-5, arch="mpnet", pooling="mean", normalize=True)
#: all-MiniLM-L6-v2 geometry (BERT, hidden 384, 12 heads of 32, mean pooling + Normalize); synthetic-weight runs
#: override num_layers / pooling as needed
BERT_SMALL_CFG = dict(num_layers=6, hidden=384, heads=12, ffn=1536, vocab=30522, max_pos=512, rel_buckets=0,
                      pad_id=0, max_seq_len=512, ln_eps=1e-12, arch="bert", pooling="mean", normalize=True)
#: bge-base-en-v1.5 geometry (BERT, hidden 768, 12 heads of 64, CLS pooling + Normalize)
BERT_BASE_CFG = dict(BERT_SMALL_CFG, num_layers=12, hidden=768, ffn=3072, pooling="cls")

_ARCH_ID = {"mpnet": 0, "bert": 1}
_POOL_ID = {"mean": 0, "cls": 1}
_KERNEL_LIMIT_SEQ = 512
_ST_MODULES = {"sentence_transformers.models.Transformer": "transformer",
               "sentence_transformers.models.Pooling": "pooling",
               "sentence_transformers.models.Normalize": "normalize"}


def _pooling_mode(pcfg: dict) -> str:
    """mean / cls from a sentence-transformers ``Pooling`` config; any other mode raises ``ValueError`` naming it."""
    if "pooling_mode" in pcfg and isinstance(pcfg["pooling_mode"], str):   # (the short form some versions write)
        mode = pcfg["pooling_mode"]
        if mode not in ("mean", "cls"):
            raise ValueError(f"unsupported pooling mode: pooling_mode={mode!r} (supported: 'mean', 'cls')")
        return mode
    on = sorted(k for k, v in pcfg.items() if k.startswith("pooling_mode_") and v)
    bad = [k for k in on if k not in ("pooling_mode_mean_tokens", "pooling_mode_cls_token")]
    if bad:
        raise ValueError(f"unsupported pooling mode: {', '.join(bad)} (supported: pooling_mode_mean_tokens, "
                         "pooling_mode_cls_token)")
    if len(on) != 1:
        raise ValueError(f"pooling config must enable exactly one of pooling_mode_mean_tokens / pooling_mode_cls_token "
                         f"(enabled: {on or 'none'})")
    return "mean" if on[0] == "pooling_mode_mean_tokens" else "cls"


def parse_model_config(model_dir: Union[str, Path]) -> dict:
    """The encoder configuration of a checkpoint directory (no GPU needed): ``config.json`` of the transformer
    (``model_type`` mpnet or bert, ``hidden_act`` gelu, geometry, ``layer_norm_eps``, ``pad_token_id``,
    ``max_position_embeddings``) plus the sentence-transformers modules: the pooling mode from ``1_Pooling/config.json``
    (mean or CLS) and whether a ``Normalize`` module follows (``modules.json``).  A directory without ``modules.json`` is
    taken as Transformer + mean Pooling + Normalize (the all-mpnet-base-v2 pipeline).  Anything the kernels do not
    implement raises ``ValueError`` naming the field."""
    model_dir = Path(model_dir)
    root = model_dir / "0_Transformer" if (model_dir / "0_Transformer").is_dir() else model_dir
    hf = json.loads((root / "config.json").read_text())
    model_type = hf.get("model_type", "mpnet")
    if model_type not in _ARCH_ID:
        raise ValueError(f"unsupported model_type {model_type!r} (supported: 'mpnet', 'bert')")
    act = hf.get("hidden_act", "gelu")
    if act != "gelu":
        raise ValueError(f"unsupported hidden_act {act!r} (the encoder implements the exact erf 'gelu')")
    bert = model_type == "bert"
    hidden, heads = int(hf.get("hidden_size", 768)), int(hf.get("num_attention_heads", 12))
    if heads < 1 or hidden % heads:
        raise ValueError(f"hidden_size {hidden} is not a multiple of num_attention_heads {heads}")
    head_dim = hidden // heads
    if bert:
        if hidden not in (384, 768):
            raise ValueError(f"unsupported hidden_size {hidden} for model_type 'bert' (supported: 384, 768)")
        if head_dim not in (32, 64):
            raise ValueError(f"unsupported head_dim {head_dim} (hidden_size / num_attention_heads) for model_type "
                             "'bert' (supported: 32, 64)")
        if int(hf.get("type_vocab_size", 2)) != 2:
            raise ValueError(f"unsupported type_vocab_size {hf['type_vocab_size']} (supported: 2)")
        pet = hf.get("position_embedding_type", "absolute")
        if pet != "absolute":
            raise ValueError(f"unsupported position_embedding_type {pet!r} (supported: 'absolute')")
    elif hidden != 768 or head_dim != 64:
        raise ValueError(f"unsupported geometry for model_type 'mpnet': hidden_size {hidden}, head_dim {head_dim} "
                         "(supported: 768, 64)")
    max_pos = int(hf.get("max_position_embeddings", 512 if bert else 514))
    cfg = dict(DEFAULT_CFG)
    cfg.update(num_layers=int(hf.get("num_hidden_layers", 12)), hidden=hidden, heads=heads,
               ffn=int(hf.get("intermediate_size", 4 * hidden)), vocab=int(hf.get("vocab_size", 30522 if bert else 30527)),
               max_pos=max_pos, rel_buckets=int(hf.get("relative_attention_num_buckets", 0 if bert else 32)),
               pad_id=int(hf.get("pad_token_id", 0 if bert else 1)),
               ln_eps=float(hf.get("layer_norm_eps", 1e-12 if bert else 1e-5)), arch=model_type)
    if bert:
        cfg["max_seq_len"] = min(max_pos, _KERNEL_LIMIT_SEQ)
    # sentence-transformers modules
    mods_file = model_dir / "modules.json"
    if mods_file.is_file():
        mods = sorted(json.loads(mods_file.read_text()), key=lambda m: int(m.get("idx", 0)))
        kinds = []
        for m in mods:
            kind = _ST_MODULES.get(m.get("type", ""))
            if kind is None:
                raise ValueError(f"unsupported sentence-transformers module {m.get('type')!r} in modules.json (supported: "
                                 "Transformer, Pooling, Normalize)")
            kinds.append(kind)
        if kinds not in (["transformer", "pooling"], ["transformer", "pooling", "normalize"]):
            raise ValueError(f"unsupported module list in modules.json: {kinds} (supported: Transformer, Pooling "
                             "[, Normalize])")
        pdir = model_dir / mods[1].get("path", "1_Pooling")
        pcfg = json.loads((pdir / "config.json").read_text()) if (pdir / "config.json").is_file() else {}
        cfg["pooling"] = _pooling_mode(pcfg) if pcfg else "mean"
        wdim = pcfg.get("word_embedding_dimension")
        if wdim is not None and int(wdim) != hidden:
            raise ValueError(f"Pooling word_embedding_dimension {wdim} differs from hidden_size {hidden}")
        cfg["normalize"] = kinds[-1] == "normalize"
    return cfg


def _is_model_dir(c: Path) -> bool:
    return c.is_dir() and ((c / "config.json").exists() or (c / "0_Transformer").is_dir())


def _hub_snapshots(root: Path, name: str) -> List[Path]:
    """Snapshot directories of the HF-hub cache layout ``root/models--<org>--<name>/snapshots/<rev>/`` -- where
    sentence-transformers >= 3 (the reference pins >= 5, ``pyproject.toml``) leaves an auto-downloaded model when it
    is given ``cache_folder`` (``src/embeddings.py:81-88``).  ``refs/main`` names the current revision; otherwise
    the most recently modified snapshot wins."""
    org, _, base = name.rpartition("/")
    repos = [f"models--{org.replace('/', '--')}--{base}"] if org else [f"models--sentence-transformers--{base}", f"models--{base}"]
    out: List[Path] = []
    for repo in repos:
        snaps = root / repo / "snapshots"
        if not snaps.is_dir():
            continue
        ref = root / repo / "refs" / "main"
        if ref.is_file():
            cand = snaps / ref.read_text().strip()
            if cand.is_dir():
                out.append(cand)
        out += sorted((d for d in snaps.iterdir() if d.is_dir()), key=lambda d: -d.stat().st_mtime)
    return out


def _find_model_dir(name_or_path: str, cache_folder: Optional[str]) -> Optional[Path]:
    """Where ``SentenceTransformer(name, cache_folder=...)`` would find the model without a network: the path itself,
    the flat layouts ``<cache>/<name>`` and ``<cache>/sentence-transformers_<name>`` (what the reference's
    ``scripts/model_setup.py:38-52`` writes), and the HF-hub layout under ``cache_folder``,
    ``$SENTENCE_TRANSFORMERS_HOME``, ``$HF_HUB_CACHE`` / ``$HF_HOME/hub`` and ``~/.cache/huggingface/hub``."""
    cands: List[Path] = [Path(name_or_path)]
    base = name_or_path.rpartition("/")[2]
    roots: List[Path] = []
    if cache_folder:
        roots.append(Path(cache_folder))
    home = os.environ.get("SENTENCE_TRANSFORMERS_HOME")
    if home:
        roots.append(Path(home))
    hub_roots = list(roots)
    if os.environ.get("HF_HUB_CACHE"):
        hub_roots.append(Path(os.environ["HF_HUB_CACHE"]))
    if os.environ.get("HF_HOME"):
        hub_roots.append(Path(os.environ["HF_HOME"]) / "hub")
    hub_roots.append(Path.home() / ".cache" / "huggingface" / "hub")
    for r in roots:
        cands += [r / name_or_path, r / base, r / f"sentence-transformers_{base}"]
    for r in hub_roots:
        cands += _hub_snapshots(r, name_or_path)
    for c in cands:
        if _is_model_dir(c):
            return c
    return None


def _tokenizer_files(model_dir: Path) -> Dict[str, object]:
    """``vocab.txt`` and the lower-casing flag of a checkpoint directory.  Modern sentence-transformers layouts keep the
    tokenizer files at the ROOT beside ``modules.json`` even when the weights sit in ``0_Transformer/``; older ones
    keep everything in ``0_Transformer/``.  ``do_lower_case`` comes from ``tokenizer_config.json`` (all-mpnet-base-v2:
    true -- MPNetTokenizer lower-cases; the ``do_lower_case: false`` of ``sentence_bert_config.json`` only says that
    sentence-transformers does not lower-case a second time)."""
    places = [model_dir, model_dir / "0_Transformer"]
    vocab = next((p / "vocab.txt" for p in places if (p / "vocab.txt").is_file()), None)
    lower = True
    for p in places:
        f = p / "tokenizer_config.json"
        if f.is_file():
            lower = bool(json.loads(f.read_text()).get("do_lower_case", True))
            break
    max_len = None
    for p in places:
        f = p / "sentence_bert_config.json"
        if f.is_file():
            max_len = json.loads(f.read_text()).get("max_seq_length")
            break
    return {"vocab": vocab, "lower": lower, "max_seq_length": max_len}


def _load_state_dict(model_dir: Path) -> Dict[str, np.ndarray]:
    sub = model_dir / "0_Transformer"
    root = sub if sub.is_dir() else model_dir
    st = root / "model.safetensors"
    if st.exists():
        from safetensors.numpy import load_file

        return {k: np.asarray(v, dtype=np.float32) for k, v in load_file(str(st)).items()}
    pt = root / "pytorch_model.bin"
    if pt.exists():
        import torch

        sd = torch.load(str(pt), map_location="cpu", weights_only=True)
        return {k: v.float().numpy() for k, v in sd.items()}
    raise FileNotFoundError(f"no model.safetensors / pytorch_model.bin under {root}")


class MpnetEncoder:
    def __init__(self, model_name_or_path: Optional[str] = "all-mpnet-base-v2", cache_folder: Optional[str] = None,
                 device: int = 0, compute: str = "bf16", synthetic_seed: Optional[int] = None,
                 cfg_overrides: Optional[dict] = None, weights: Optional[Dict[str, np.ndarray]] = None):
        # weights: a state dict to load in place of the checkpoint's own file (CrossEncoder passes the body of a
        # sequence-classification checkpoint, whose head tensors the strict loader does not know)
        cfg = dict(DEFAULT_CFG)
        model_dir = None
        if synthetic_seed is None:
            model_dir = _find_model_dir(model_name_or_path or "", cache_folder)
            if model_dir is None:
                raise FileNotFoundError(
                    f"model '{model_name_or_path}' not found locally (no network): pass a directory in HF layout, "
                    "or synthetic_seed=<int> for seeded synthetic weights"
                )
            cfg = parse_model_config(model_dir)
        if cfg_overrides:
            cfg.update(cfg_overrides)
        if cfg["arch"] not in _ARCH_ID or cfg["pooling"] not in _POOL_ID:
            raise ValueError(f"arch must be one of {sorted(_ARCH_ID)} and pooling one of {sorted(_POOL_ID)}")
        self.cfg = cfg
        self._device_index = int(device)
        self.compute = compute
        c = nat.EncoderCfg(cfg["num_layers"], cfg["hidden"], cfg["heads"], cfg["ffn"], cfg["vocab"], cfg["max_pos"],
                           cfg["rel_buckets"], cfg["pad_id"], cfg["max_seq_len"], cfg["ln_eps"],
                           0 if compute == "bf16" else 1, _ARCH_ID[cfg["arch"]], _POOL_ID[cfg["pooling"]])
        h = ctypes.c_void_p()
        nat.check(nat.lib().css_encoder_create(ctypes.byref(c), self._device_index, ctypes.byref(h)))
        self._h = h
        self.max_seq_length = cfg["max_seq_len"]
        self.model_dir = model_dir
        #: why text cannot be encoded (None when it can); surfaced by EmbeddingGenerator.get_model_info()
        self.tokenizer_problem: Optional[str] = None
        if synthetic_seed is not None:
            nat.check(nat.lib().css_encoder_init_synthetic(self._h, ctypes.c_uint64(synthetic_seed)))
            self.tokenizer = HashTokenizer(cfg["vocab"])   # synthetic weights: any deterministic text -> ids map will do
        else:
            self.load_state_dict(_load_state_dict(model_dir) if weights is None else weights)
            tk = _tokenizer_files(model_dir)
            if tk["max_seq_length"]:
                self.max_seq_length = min(int(tk["max_seq_length"]), cfg["max_seq_len"])
            if tk["vocab"] is not None:
                self.tokenizer = make_wordpiece(str(tk["vocab"]), lower=bool(tk["lower"]))
            else:
                # REAL weights with word ids from a hash would give plausible-looking garbage: refuse text instead
                self.tokenizer = None
                self.tokenizer_problem = (f"checkpoint {model_dir} has no vocab.txt (looked beside config.json and in "
                                          "0_Transformer/): text cannot be tokenised for these weights")
                logging.getLogger(__name__).warning(self.tokenizer_problem + "; encode_ids() still works")

    # -- lifetime -----------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            nat.lib().css_encoder_free(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # -- weights ------------------------------------------------------------
    def load_state_dict(self, sd: Dict[str, np.ndarray]) -> None:
        names = [k for k in sd if "pooler." not in k and "position_ids" not in k and "token_type_ids" not in k]
        arr = (nat.Tensor * len(names))()
        keep = []
        for i, k in enumerate(names):
            a = np.ascontiguousarray(sd[k], dtype=np.float32)
            keep.append(a)
            arr[i].name = k.encode()
            arr[i].data = a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
            arr[i].numel = a.size
        nat.check(nat.lib().css_encoder_load_weights(self._h, arr, len(names)))

    def export_weight(self, name: str, shape) -> np.ndarray:
        out = np.empty(shape, dtype=np.float32)
        nat.check(nat.lib().css_encoder_export_weight(self._h, name.encode(), out.ctypes.data, out.size))
        return out

    def set_attention_range(self, value: float) -> None:
        """Verification knob of the bf16 attention kernel (``css_encoder_set_attention_range``): 0 forces the
        running-maximum softmax pass, the default 2**100 keeps the reference-free pass while row sums fit fp32."""
        nat.check(nat.lib().css_encoder_set_attention_range(self._h, ctypes.c_float(value)))

    def debug_read(self, what: str, shape) -> np.ndarray:
        out = np.empty(shape, dtype=np.float32)
        nat.check(nat.lib().css_encoder_debug_read(self._h, what.encode(), out.ctypes.data, out.size))
        return out

    # -- SentenceTransformer surface ------------------------------------------
    def to(self, device) -> "MpnetEncoder":
        return self  # the model already lives on its HIP device

    @property
    def device(self) -> str:
        return f"cuda:{self._device_index}"  # the name PyTorch-ROCm gives a HIP device

    def get_sentence_embedding_dimension(self) -> int:
        return int(self.cfg["hidden"])

    def tokenize(self, texts: Sequence[str]) -> List[List[int]]:
        if self.tokenizer is None:
            raise RuntimeError(self.tokenizer_problem or "no tokenizer")
        L = min(int(self.max_seq_length), int(self.cfg["max_seq_len"]))
        if hasattr(self.tokenizer, "encode_batch"):
            return self.tokenizer.encode_batch(texts, L)
        return [self.tokenizer.encode(t, L) for t in texts]

    def encode_ids(self, batch: Sequence[Sequence[int]], normalize: bool = True) -> np.ndarray:
        """One packed var-len batch through ``css_encoder_forward``."""
        B = len(batch)
        lens = np.fromiter((len(s) for s in batch), dtype=np.int32, count=B)
        cu = np.zeros(B + 1, dtype=np.int32)
        np.cumsum(lens, out=cu[1:])
        ids = np.concatenate([np.asarray(s, dtype=np.int32) for s in batch]) if B else np.zeros(0, np.int32)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        out = np.empty((B, self.cfg["hidden"]), dtype=np.float32)
        nat.check(nat.lib().css_encoder_forward(self._h, ids.ctypes.data, cu.ctypes.data, B, 1 if normalize else 0,
                                                out.ctypes.data))
        return out

    def encode_spans_ids(self, batch: Sequence[Sequence[int]], spans, normalize: bool = True, query=None,
                         span_rows: bool = True):
        """One packed var-len batch through ``css_encoder_forward_spans``: the forward pass of ``encode_ids`` plus one
        pooled row per span ``(sequence, begin, end)`` (token positions relative to the sequence) -- the masked MEAN of
        the final hidden states of tokens ``begin..end-1``, also for a CLS-pooling model.  Returns
        ``(seq_emb [B, hidden], span_emb [S, hidden], scores [S] | None)``; ``scores`` (with ``query`` [hidden]) are
        ``dot(query, span row)`` formed on the device.  ``seq_emb`` is exactly what ``encode_ids`` returns.
        ``span_rows=False`` (scores only) leaves the span rows on the device and returns ``None`` for them."""
        B = len(batch)
        H = int(self.cfg["hidden"])
        lens = np.fromiter((len(s) for s in batch), dtype=np.int32, count=B)
        cu = np.zeros(B + 1, dtype=np.int32)
        np.cumsum(lens, out=cu[1:])
        ids = np.concatenate([np.asarray(s, dtype=np.int32) for s in batch]) if B else np.zeros(0, np.int32)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        sp = np.ascontiguousarray(np.asarray(spans if len(spans) else np.zeros((0, 3)), dtype=np.int64))
        if sp.ndim != 2 or sp.shape[1] != 3:
            raise ValueError(f"encode_spans_ids: spans must be [S, 3] = (sequence, begin, end) (got shape {sp.shape})")
        if sp.size and np.abs(sp).max() >= 2 ** 31:
            raise ValueError("encode_spans_ids: span entries must fit int32")
        sp = np.ascontiguousarray(sp, dtype=np.int32)
        S = int(sp.shape[0])
        q = None
        if query is not None:
            q = np.ascontiguousarray(query, dtype=np.float32).reshape(-1)
            if q.size != H:
                raise ValueError(f"encode_spans_ids: query has {q.size} elements, the model's hidden size is {H}")
        seq = np.empty((B, H), dtype=np.float32)
        out = np.empty((S, H), dtype=np.float32) if span_rows else None
        scores = np.empty(S, dtype=np.float32) if q is not None else None
        nat.check(nat.lib().css_encoder_forward_spans(
            self._h, ids.ctypes.data, cu.ctypes.data, B, sp.ctypes.data if S else None, S,
            q.ctypes.data if q is not None else None, 1 if normalize else 0, seq.ctypes.data,
            out.ctypes.data if out is not None else None,
            scores.ctypes.data if scores is not None else None))
        return seq, out, scores

    # -- cross-encoder head ----------------------------------------------------
    def set_head(self, pooler_w, pooler_b, cls_w, cls_b) -> None:
        """The sequence-classification head of a BERT cross-encoder (``css_encoder_set_head``): ``pooler_w`` [H, H],
        ``pooler_b`` [H], ``cls_w`` [H] or [1, H], ``cls_b`` [1].  May be called again to replace the head."""
        H = int(self.cfg["hidden"])
        arrs = []
        for name, a, shapes in (("pooler_w", pooler_w, ((H, H),)), ("pooler_b", pooler_b, ((H,),)),
                                ("cls_w", cls_w, ((H,), (1, H))), ("cls_b", cls_b, ((1,), ()))):
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape not in shapes:
                raise ValueError(f"set_head: {name} has shape {a.shape}, expected {' or '.join(map(str, shapes))}")
            arrs.append(a.reshape(-1))
        nat.check(nat.lib().css_encoder_set_head(self._h, *(a.ctypes.data for a in arrs)))

    def score_pair_ids(self, batch: Sequence[Sequence[int]], seg_starts: Sequence[int]) -> np.ndarray:
        """One packed var-len batch of ``[CLS] a [SEP] b [SEP]`` sequences through ``css_encoder_forward_pairs``:
        tokens at positions ``< seg_starts[b]`` take token type 0, the others type 1.  Returns the float32 logits [B]."""
        B = len(batch)
        seg = np.asarray(seg_starts, dtype=np.int64).reshape(-1)
        if seg.size != B:
            raise ValueError(f"score_pair_ids: {seg.size} seg_starts for {B} sequences")
        if B == 0:
            return np.zeros(0, dtype=np.float32)
        if np.abs(seg).max() >= 2 ** 31:
            raise ValueError("score_pair_ids: seg_starts must fit int32")
        seg = np.ascontiguousarray(seg, dtype=np.int32)
        lens = np.fromiter((len(s) for s in batch), dtype=np.int32, count=B)
        cu = np.zeros(B + 1, dtype=np.int32)
        np.cumsum(lens, out=cu[1:])
        ids = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.int32) for s in batch]), dtype=np.int32)
        out = np.empty(B, dtype=np.float32)
        nat.check(nat.lib().css_encoder_forward_pairs(self._h, ids.ctypes.data, cu.ctypes.data, seg.ctypes.data, B,
                                                      out.ctypes.data))
        return out

    # -- late interaction: token vectors and MaxSim ------------------------------
    def set_token_projection(self, W) -> None:
        """The bias-free token projection of a ColBERT checkpoint (``css_encoder_set_token_projection``): ``W`` [P, H]
        with P a multiple of 32 in [32, 128]; ``None`` clears it (the token vectors are then the hidden states)."""
        if W is None:
            nat.check(nat.lib().css_encoder_set_token_projection(self._h, None, 0))
            return
        H = int(self.cfg["hidden"])
        W = np.ascontiguousarray(W, dtype=np.float32)
        if W.ndim != 2 or W.shape[1] != H:
            raise ValueError(f"set_token_projection: W has shape {W.shape}, expected [P, {H}]")
        nat.check(nat.lib().css_encoder_set_token_projection(self._h, W.ctypes.data, int(W.shape[0])))

    @property
    def token_dim(self) -> int:
        """Columns of a token vector: the projection's P, or the hidden size without one."""
        return int(nat.lib().css_encoder_token_dim(self._h))

    @staticmethod
    def _pack_ids(batch: Sequence[Sequence[int]]):
        B = len(batch)
        lens = np.fromiter((len(s) for s in batch), dtype=np.int32, count=B)
        cu = np.zeros(B + 1, dtype=np.int32)
        np.cumsum(lens, out=cu[1:])
        ids = np.concatenate([np.asarray(s, dtype=np.int32) for s in batch]) if B else np.zeros(0, np.int32)
        return np.ascontiguousarray(ids, dtype=np.int32), cu

    @staticmethod
    def _pack_mats(name: str, mats, P: Optional[int] = None):
        """``(rows [sum m, P] uint16, cu [n + 1] int32, P)`` of a list of bf16 token matrices (uint16 bit patterns)."""
        mats = [np.asarray(m) for m in mats]
        for i, m in enumerate(mats):
            if m.dtype != np.uint16 or m.ndim != 2:
                raise ValueError(f"{name}[{i}] must be a uint16 [tokens, P] matrix of bf16 bit patterns "
                                 f"(got dtype {m.dtype}, shape {m.shape})")
            if P is None:
                P = int(m.shape[1])
            if m.shape[1] != P:
                raise ValueError(f"{name}[{i}] has P={m.shape[1]} columns, expected P={P}")
        cu = np.zeros(len(mats) + 1, dtype=np.int32)
        np.cumsum([m.shape[0] for m in mats], out=cu[1:])
        rows = np.ascontiguousarray(np.concatenate(mats, axis=0)) if mats else np.zeros((0, P or 0), np.uint16)
        return rows, cu, P

    @staticmethod
    def _pack_pairs(pairs, nq: int, nd: int) -> np.ndarray:
        if pairs is None:   # every query against every doc, query-major
            pairs = [(i, j) for i in range(nq) for j in range(nd)]
        pr = np.asarray(pairs if len(pairs) else np.zeros((0, 2)), dtype=np.int64)
        if pr.ndim != 2 or pr.shape[1] != 2:
            raise ValueError(f"pairs must be [np, 2] = (query, doc) (got shape {pr.shape})")
        if pr.size and np.abs(pr).max() >= 2 ** 31:
            raise ValueError("pair entries must fit int32")
        return np.ascontiguousarray(pr, dtype=np.int32)

    @staticmethod
    def _pack_keep(keep, cu_d: np.ndarray) -> Optional[np.ndarray]:
        if keep is None:
            return None
        flat = np.concatenate([np.asarray(k).reshape(-1) != 0 for k in keep]) if len(keep) else np.zeros(0, bool)
        lens = [int(np.asarray(k).size) for k in keep]
        if lens != list(np.diff(cu_d)):
            raise ValueError("keep must hold one flag per doc token (lengths differ from the docs')")
        return np.ascontiguousarray(flat, dtype=np.uint8)

    def encode_tokens_ids(self, batch: Sequence[Sequence[int]], normalize: bool = True, return_seq: bool = False):
        """One packed var-len batch through ``css_encoder_forward_tokens``: per sequence its token matrix, uint16
        [len_b, P] of bf16 bit patterns (``W h_t`` or ``h_t``, unit rows when ``normalize``).  ``return_seq=True`` also
        returns what ``encode_ids`` returns for the batch."""
        ids, cu = self._pack_ids(batch)
        B, P = len(batch), self.token_dim
        tok = np.empty((int(cu[-1]), P), dtype=np.uint16)
        seq = np.empty((B, int(self.cfg["hidden"])), dtype=np.float32) if return_seq else None
        nat.check(nat.lib().css_encoder_forward_tokens(self._h, ids.ctypes.data, cu.ctypes.data, B, 1 if normalize else 0,
                                                       tok.ctypes.data, seq.ctypes.data if seq is not None else None))
        mats = [tok[cu[b]:cu[b + 1]] for b in range(B)]
        return (mats, seq) if return_seq else mats

    def maxsim(self, q_mats, d_mats, pairs=None, keep=None) -> np.ndarray:
        """``css_encoder_maxsim`` over kept token matrices (no forward pass): float32 scores, one per ``(query, doc)``
        pair (``pairs=None``: every query against every doc, query-major).  ``keep``: per doc one flag per token, or
        ``None``."""
        q, cu_q, P = self._pack_mats("q_mats", q_mats)
        d, cu_d, P = self._pack_mats("d_mats", d_mats, P)
        pr = self._pack_pairs(pairs, len(q_mats), len(d_mats))
        kp = self._pack_keep(keep, cu_d)
        out = np.empty(pr.shape[0], dtype=np.float32)
        nat.check(nat.lib().css_encoder_maxsim(self._h, q.ctypes.data, cu_q.ctypes.data, len(q_mats), d.ctypes.data,
                                               cu_d.ctypes.data, len(d_mats), kp.ctypes.data if kp is not None else None,
                                               pr.ctypes.data, int(pr.shape[0]), int(P or 0), out.ctypes.data))
        return out

    def score_late_ids(self, batch: Sequence[Sequence[int]], q_mats, pairs=None, keep=None, return_tokens: bool = False):
        """One packed var-len batch of documents through ``css_encoder_forward_maxsim``: unit token vectors of the
        batch, then MaxSim of ``q_mats`` against the batch's sequences, in one call.  Returns the float32 scores (with
        ``return_tokens=True`` also the token matrices)."""
        ids, cu = self._pack_ids(batch)
        B, P = len(batch), self.token_dim
        q, cu_q, _ = self._pack_mats("q_mats", q_mats, P)
        pr = self._pack_pairs(pairs, len(q_mats), B)
        kp = self._pack_keep(keep, cu)
        out = np.empty(pr.shape[0], dtype=np.float32)
        tok = np.empty((int(cu[-1]), P), dtype=np.uint16) if return_tokens else None
        nat.check(nat.lib().css_encoder_forward_maxsim(self._h, ids.ctypes.data, cu.ctypes.data, B, q.ctypes.data,
                                                       cu_q.ctypes.data, len(q_mats),
                                                       kp.ctypes.data if kp is not None else None, pr.ctypes.data,
                                                       int(pr.shape[0]), out.ctypes.data,
                                                       tok.ctypes.data if tok is not None else None))
        if return_tokens:
            return out, [tok[cu[b]:cu[b + 1]] for b in range(B)]
        return out

    # -- learned sparse encoding: masked-LM head and vocabulary maximum -------------
    def set_mlm_head(self, dense_w, dense_b, ln_g, ln_b, decoder_w, decoder_b) -> None:
        """The masked-LM head of a ``BertForMaskedLM`` (``css_encoder_set_mlm_head``): ``dense_w`` [H, H], ``dense_b``
        [H], ``ln_g`` / ``ln_b`` [H], ``decoder_w`` [V, H] or ``None`` (tied to the word embeddings as loaded),
        ``decoder_b`` [V].  May be called again to replace the head."""
        H, V = int(self.cfg["hidden"]), int(self.cfg["vocab"])
        arrs = []
        for name, a, shape in (("dense_w", dense_w, (H, H)), ("dense_b", dense_b, (H,)), ("ln_g", ln_g, (H,)),
                               ("ln_b", ln_b, (H,)), ("decoder_w", decoder_w, (V, H)), ("decoder_b", decoder_b, (V,))):
            if a is None and name == "decoder_w":
                arrs.append(None)
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != shape:
                raise ValueError(f"set_mlm_head: {name} has shape {a.shape}, expected {shape}")
            arrs.append(a)
        nat.check(nat.lib().css_encoder_set_mlm_head(self._h, *(a.ctypes.data if a is not None else None for a in arrs)))

    def encode_sparse_ids(self, batch: Sequence[Sequence[int]], m: int, return_dense: bool = False,
                          return_rows: bool = False):
        """One packed var-len batch through ``css_encoder_forward_sparse``: ``(terms int32 [B, m], weights float32
        [B, m], nnz int32 [B])`` -- per sequence its ``m`` heaviest vocabulary terms, best first, padded with -1 / 0, and
        the number of positive terms before the cut.  ``return_dense=True`` appends ``z`` [B, V] (the maxima before
        ``log1p``), ``return_rows=True`` the head's token rows ``g`` [tokens, H] (fp32, before the bf16 rounding)."""
        ids, cu = self._pack_ids(batch)
        B, m = len(batch), int(m)
        terms = np.empty((B, m), dtype=np.int32)
        weights = np.empty((B, m), dtype=np.float32)
        nnz = np.empty(B, dtype=np.int32)
        dense = np.empty((B, int(self.cfg["vocab"])), dtype=np.float32) if return_dense else None
        rows = np.empty((int(cu[-1]), int(self.cfg["hidden"])), dtype=np.float32) if return_rows else None
        nat.check(nat.lib().css_encoder_forward_sparse(self._h, ids.ctypes.data, cu.ctypes.data, B, m, terms.ctypes.data,
                                                       weights.ctypes.data, nnz.ctypes.data,
                                                       dense.ctypes.data if dense is not None else None,
                                                       rows.ctypes.data if rows is not None else None))
        out = (terms, weights, nnz)
        if return_dense:
            out += (dense,)
        if return_rows:
            out += (rows,)
        return out

    def vocab_max(self, rows, cu) -> np.ndarray:
        """``css_encoder_vocab_max`` (no forward pass): ``z`` [B, V] of the token rows ``rows`` [tokens, H] (taken as the
        head's ``g``) split into sequences by the offsets ``cu`` [B + 1]."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        cu = np.ascontiguousarray(cu, dtype=np.int32).reshape(-1)
        H = int(self.cfg["hidden"])
        if rows.ndim != 2 or rows.shape[1] != H:
            raise ValueError(f"vocab_max: rows has shape {rows.shape}, expected [tokens, {H}]")
        if cu.size < 2 or int(cu[-1]) != rows.shape[0]:
            raise ValueError(f"vocab_max: cu must hold B + 1 >= 2 offsets ending at the row count {rows.shape[0]}")
        B = cu.size - 1
        out = np.empty((B, int(self.cfg["vocab"])), dtype=np.float32)
        nat.check(nat.lib().css_encoder_vocab_max(self._h, rows.ctypes.data, cu.ctypes.data, B, out.ctypes.data))
        return out

    def best_passages(self, query_vec, texts: Sequence[str], n: int = 1, min_tokens: int = 8, max_tokens: int = 64,
                      normalize: bool = True):
        """``List[List[Passage]]``: per text its ``n`` best passages against ``query_vec``, best first, ties by position
        (``passages.best_passages``: split at sentence and line ends, packed, one ``encode_spans_ids`` call)."""
        from .passages import best_passages

        return best_passages(self, query_vec, texts, n=n, min_tokens=min_tokens, max_tokens=max_tokens, normalize=normalize)

    def encode(self, sentences: Union[str, Sequence[str]], batch_size: int = 32, normalize_embeddings: bool = False,
               show_progress_bar: bool = False, convert_to_numpy: bool = True, **_ignored) -> np.ndarray:
        single = isinstance(sentences, str)
        texts = [sentences] if single else list(sentences)
        if not texts:
            return np.zeros((0, self.cfg["hidden"]), dtype=np.float32)
        out = np.empty((len(texts), self.cfg["hidden"]), dtype=np.float32)
        bs = max(1, int(batch_size))
        norm = bool(self.cfg.get("normalize", True) or normalize_embeddings)
        # Super-batches of 16 device batches: the next one is tokenised on a host thread (both the C++ tokenizer and
        # the forward release the GIL) while the GPU encodes the current one; texts are length-sorted inside a
        # super-batch (packed var-len batches have no padding, sorting only keeps a batch's attention tiles even).
        span = max(16 * bs, 1024)
        starts = list(range(0, len(texts), span))
        bar = None
        if show_progress_bar:
            try:
                from tqdm import tqdm

                bar = tqdm(total=(len(texts) + bs - 1) // bs, desc="Batches")
            except Exception:
                bar = None
        def run(base: int, toks) -> None:
            order = sorted(range(len(toks)), key=lambda i: -len(toks[i]))
            for s in range(0, len(order), bs):
                idx = order[s:s + bs]
                # a Normalize() module of the model makes outputs unit norm regardless of the flag
                out[[base + i for i in idx]] = self.encode_ids([toks[i] for i in idx], normalize=norm)
                if bar is not None:
                    bar.update(1)

        if len(starts) == 1:  # (the single-query path: no thread hop)
            run(0, self.tokenize(texts))
        else:
            from concurrent.futures import ThreadPoolExecutor

            with ThreadPoolExecutor(max_workers=1) as pool:
                fut = pool.submit(self.tokenize, texts[:span])
                for si, base in enumerate(starts):
                    toks = fut.result()
                    if si + 1 < len(starts):
                        fut = pool.submit(self.tokenize, texts[starts[si + 1]:starts[si + 1] + span])
                    run(base, toks)
        if bar is not None:
            bar.close()
        return out[0] if single else out
