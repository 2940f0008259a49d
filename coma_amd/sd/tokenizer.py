"""Dependency-free CLIP BPE tokenizer: the surface of transformers' ``CLIPTokenizer`` that the pipeline's ``_encode_prompt`` uses
(``from_pretrained(tokenizer_dir)``, ``model_max_length``, ``__call__(prompts, padding="max_length", max_length=..., truncation=True,
return_tensors="pt").input_ids``), with the same ids.

What CLIPTokenizer does, step by step: NFC, every whitespace run -> one space, lower case; split with CLIP's pattern
``<|startoftext|>|<|endoftext|>|'s|'t|'re|'ve|'m|'ll|'d|[\\p{L}]+|[\\p{N}]|[^\\s\\p{L}\\p{N}]+`` (whitespace dropped); map every piece's
UTF-8 bytes to GPT-2's printable byte symbols, mark its last symbol with ``</w>`` and merge by rank (merges.txt); BOS + ids + EOS,
truncated to max_length (EOS kept), padded with the pad token.  Letters and digits are classified with ``unicodedata`` categories
(L*, N*) in a small scanner instead of the ``regex`` module.
"""
from __future__ import annotations

import json
import os
import unicodedata

import torch

SPECIALS = ("<|startoftext|>", "<|endoftext|>")
CONTRACTIONS = ("s", "t", "re", "ve", "m", "ll", "d")


def bytes_to_unicode():
    """GPT-2 / CLIP byte -> printable symbol table (printable Latin-1 bytes map to themselves, the rest to 256 + n)."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, map(chr, cs)))


def _is_letter(ch):
    return unicodedata.category(ch)[0] == "L"


def _is_number(ch):
    return unicodedata.category(ch)[0] == "N"


def normalize(text):
    """NFC, whitespace runs collapsed to one space and stripped, lower-cased."""
    text = unicodedata.normalize("NFC", text)
    return " ".join(text.split()).lower()


def pre_tokenize(text):
    """CLIP's split pattern as a scanner over normalised text: alternatives tried in the pattern's order at every position."""
    out, i, n = [], 0, len(text)
    while i < n:
        ch = text[i]
        if ch.isspace():
            i += 1
            continue
        sp = next((t for t in SPECIALS if text.startswith(t, i)), None)
        if sp is not None:
            out.append(sp)
            i += len(sp)
            continue
        if ch == "'":
            c = next((c for c in CONTRACTIONS if text.startswith(c, i + 1)), None)
            if c is not None:
                out.append("'" + c)
                i += 1 + len(c)
                continue
        j = i + 1
        if _is_letter(ch):
            while j < n and _is_letter(text[j]):
                j += 1
        elif not _is_number(ch):                      # [^\s\p{L}\p{N}]+ (a single digit is a piece of its own)
            while j < n and not (text[j].isspace() or _is_letter(text[j]) or _is_number(text[j])):
                j += 1
        out.append(text[i:j])
        i = j
    return out


def _token_content(v):
    return v.get("content") if isinstance(v, dict) else v


class _Encoding(dict):
    __getattr__ = dict.__getitem__


class CLIPTokenizer:
    def __init__(self, vocab, merges, model_max_length=77, bos_token="<|startoftext|>", eos_token="<|endoftext|>", pad_token="<|endoftext|>",
                 unk_token="<|endoftext|>"):
        self.encoder = dict(vocab)
        self.bpe_ranks = {tuple(m): r for r, m in enumerate(merges)}
        self.byte_encoder = bytes_to_unicode()
        self.model_max_length = int(model_max_length)
        self.bos_token, self.eos_token, self.pad_token, self.unk_token = bos_token, eos_token, pad_token, unk_token
        for t in (bos_token, eos_token, pad_token):
            if t not in self.encoder:
                raise ValueError(f"tokenizer: special token {t!r} is not in the vocabulary")
        self.bos_token_id, self.eos_token_id = self.encoder[bos_token], self.encoder[eos_token]
        self.pad_token_id = self.encoder[pad_token]
        self.unk_token_id = self.encoder.get(unk_token, self.eos_token_id)
        self._cache = {}

    @classmethod
    def from_pretrained(cls, tokenizer_dir):
        """A checkpoint's `tokenizer/` directory: vocab.json, merges.txt and (optional) tokenizer_config.json / special_tokens_map.json."""
        d = os.fspath(tokenizer_dir)
        with open(os.path.join(d, "vocab.json"), encoding="utf-8") as f:
            vocab = json.load(f)
        with open(os.path.join(d, "merges.txt"), encoding="utf-8") as f:
            lines = f.read().split("\n")
        if lines and lines[0].startswith("#version"):
            lines = lines[1:]
        merges = [tuple(l.split()) for l in lines if len(l.split()) == 2]
        kw = {}
        for name in ("special_tokens_map.json", "tokenizer_config.json"):       # the config wins where both say something
            path = os.path.join(d, name)
            if os.path.exists(path):
                with open(path, encoding="utf-8") as f:
                    conf = json.load(f)
                for key in ("bos_token", "eos_token", "pad_token", "unk_token"):
                    if _token_content(conf.get(key)) is not None:
                        kw[key] = _token_content(conf[key])
                if isinstance(conf.get("model_max_length"), int) and conf["model_max_length"] < 1 << 30:
                    kw["model_max_length"] = conf["model_max_length"]
        return cls(vocab, merges, **kw)

    # ---- BPE
    def _bpe(self, piece):
        if piece in self._cache:
            return self._cache[piece]
        word = [self.byte_encoder[b] for b in piece.encode("utf-8")]
        word[-1] = word[-1] + "</w>"
        while len(word) > 1:
            best, at = None, -1
            for k in range(len(word) - 1):
                r = self.bpe_ranks.get((word[k], word[k + 1]))
                if r is not None and (best is None or r < best):
                    best, at = r, k
            if best is None:
                break
            pair = (word[at], word[at + 1])
            merged, k = [], 0
            while k < len(word):                      # merge every occurrence of the best pair, left to right
                if k < len(word) - 1 and (word[k], word[k + 1]) == pair:
                    merged.append(word[k] + word[k + 1])
                    k += 2
                else:
                    merged.append(word[k])
                    k += 1
            word = merged
        ids = [self.encoder.get(sym, self.unk_token_id) for sym in word]
        self._cache[piece] = ids
        return ids

    def encode(self, text, max_length=None, truncation=True):
        """BOS + token ids + EOS (truncated to max_length with EOS kept)."""
        ids = []
        for piece in pre_tokenize(normalize(text)):
            if piece in SPECIALS and piece in self.encoder:
                ids.append(self.encoder[piece])
            else:
                ids.extend(self._bpe(piece))
        if truncation and max_length is not None:
            ids = ids[:max(max_length - 2, 0)]
        return [self.bos_token_id] + ids + [self.eos_token_id]

    def __call__(self, prompts, padding="max_length", max_length=None, truncation=True, return_tensors="pt"):
        if isinstance(prompts, str):
            prompts = [prompts]
        max_length = self.model_max_length if max_length is None else int(max_length)
        rows = [self.encode(p, max_length=max_length, truncation=truncation) for p in prompts]
        if padding == "max_length":
            width = max_length
        elif padding in (True, "longest"):
            width = max(len(r) for r in rows)
        elif padding in (False, None, "do_not_pad"):
            width = None
        else:
            raise ValueError(f"padding={padding!r} is not supported")
        if width is not None:
            rows = [r + [self.pad_token_id] * (width - len(r)) for r in rows]
        if return_tensors == "pt":
            if len({len(r) for r in rows}) > 1:
                raise ValueError("rows of different lengths cannot form a tensor: pad them")
            return _Encoding(input_ids=torch.tensor(rows, dtype=torch.int64))
        if return_tensors is None:
            return _Encoding(input_ids=rows)
        raise ValueError(f"return_tensors={return_tensors!r} is not supported")
