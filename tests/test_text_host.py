"""CPU: the CLIP text tower's host side -- the dependency-free tokenizer against transformers' CLIPTokenizer, the plain-torch restatement of
CLIPTextModel (tests/clip_ref.py) against transformers, the text_encoder/ loader, and argument validation of the new C entry points (which
returns before any launch)."""
import ctypes as C
import json
import os

import pytest
import torch

from tests import clip_ref

PROMPTS = [
    clip_ref.NEGATIVE_PROMPT,
    "",
    " ".join(["a person sitting on a chair with a dog"] * 12),                 # > 77 tokens: truncated, EOS kept
    "A Person Sitting ON a CHAIR",
    "a   person\n\nsitting \t on\r\n a chair  ",
    "the person's hat, don't look, we're here, they've gone, i'm ok, you'll see, he'd go",
    "8k uhd 1080p, 3 people, 2024 photo 0.5",
    "!!! ??? ... ,,, (((masterpiece))) [best:1.2] --no #tag @me",
    "caf\u00e9 na\u00efve r\u00e9sum\u00e9, cafe\u0301 (decomposed), \u00dcn\u00efc\u00f6d\u00e9",
    "日本語のテキスト, 中文提示, русский текст, ελληνικά",
]


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("tokenizer")
    clip_ref.learn_tokenizer(str(d))
    return d


def _ids(tok, prompts):
    return tok(prompts, padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt").input_ids


def test_tokenizer_matches_transformers(tok_dir):
    transformers = pytest.importorskip("transformers")
    from coma_amd.sd.tokenizer import CLIPTokenizer
    mine = CLIPTokenizer.from_pretrained(tok_dir)
    ref = transformers.CLIPTokenizer.from_pretrained(str(tok_dir))
    assert mine.model_max_length == ref.model_max_length == 77
    for p in PROMPTS:
        a, b = _ids(mine, [p]), _ids(ref, [p])
        assert a.dtype == torch.int64 and a.shape == b.shape == (1, 77), p
        assert torch.equal(a, b), (p, a[0, :24].tolist(), b[0, :24].tolist())
    assert torch.equal(_ids(mine, PROMPTS), _ids(ref, PROMPTS))        # a batch is the rows stacked


def test_tokenizer_hand_checked_ids(tok_dir):
    """Ids that follow from the construction alone (no transformers): byte symbols are ids 0..255 in GPT-2's byte order, their `</w>`
    forms 256..511, BOS / EOS the last two entries, pad = EOS."""
    from coma_amd.sd.tokenizer import CLIPTokenizer, bytes_to_unicode
    vocab = json.loads((tok_dir / "vocab.json").read_text(encoding="utf-8"))
    tok = CLIPTokenizer.from_pretrained(tok_dir)
    bos, eos = vocab["<|startoftext|>"], vocab["<|endoftext|>"]
    assert (tok.bos_token_id, tok.eos_token_id, tok.pad_token_id) == (bos, eos, eos) == (len(vocab) - 2, len(vocab) - 1, len(vocab) - 1)
    be = bytes_to_unicode()
    byte_id = {b: vocab[be[b]] for b in range(256)}
    end_id = {b: vocab[be[b] + "</w>"] for b in range(256)}
    assert _ids(tok, [""])[0].tolist() == [bos, eos] + [eos] * 75
    # "7" and "0" are single-digit pieces, each ends a word; "?" is one piece of one byte; "q" never appears in the corpus next to z
    assert _ids(tok, ["7 0 ? zq"])[0, :7].tolist() == [bos, end_id[ord("7")], end_id[ord("0")], end_id[ord("?")],
                                                      byte_id[ord("z")], end_id[ord("q")], eos]
    # case, whitespace runs and NFC do not change the ids
    assert torch.equal(_ids(tok, ["A  PERSON\n"]), _ids(tok, ["a person"]))
    assert torch.equal(_ids(tok, ["caf\u00e9"]), _ids(tok, ["cafe\u0301"]))
    # the most frequent corpus word is one merged symbol: "quality</w>" (4 times in the negative prompt)
    assert _ids(tok, ["quality"])[0, :3].tolist() == [bos, vocab["quality</w>"], eos]
    # truncation keeps BOS ... EOS in 77 ids
    long = _ids(tok, [" ".join(["7"] * 200)])[0].tolist()
    assert len(long) == 77 and long[0] == bos and long[-1] == eos and long[1:76] == [end_id[ord("7")]] * 75


def test_tokenizer_pre_tokenisation():
    from coma_amd.sd.tokenizer import normalize, pre_tokenize
    assert pre_tokenize(normalize("Don't  stop, person's 42!!")) == ["don", "'t", "stop", ",", "person", "'s", "4", "2", "!!"]
    assert pre_tokenize("!!'s x'll") == ["!!'", "s", "x", "'ll"]                # a punctuation run takes the apostrophe first
    assert pre_tokenize("中文 ab1") == ["中文", "ab", "1"]


def test_restatement_matches_transformers():
    transformers = pytest.importorskip("transformers")
    cfg = clip_ref.small_config(layers=2, heads=2, vocab=300)
    tcfg = transformers.CLIPTextConfig(vocab_size=300, hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                                       num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77, hidden_act="quick_gelu",
                                       layer_norm_eps=1e-5, attn_implementation="eager")
    torch.manual_seed(0)
    model = transformers.CLIPTextModel(tcfg).float().eval()
    from coma_amd.sd.weights import strip_text_prefix
    state = {k: v for k, v in strip_text_prefix(model.state_dict()).items() if not k.endswith("position_ids")}
    ids = torch.randint(0, 300, (3, 77), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = model(input_ids=ids).last_hidden_state
        got = clip_ref.clip_text_ref(state, cfg, ids)
    assert got.shape == want.shape == (3, 77, cfg["hidden_size"])
    assert float((got - want).abs().max()) <= 1e-5


@pytest.mark.parametrize("prefix,fmt,dtype", [("text_model.", "safetensors", torch.float16), ("", "safetensors", torch.float32),
                                              ("text_model.", "bin", torch.float32)])
def test_loader_prefixes_formats_and_dtypes(tmp_path, prefix, fmt, dtype):
    from coma_amd.sd.weights import load_text_encoder
    cfg = clip_ref.small_config(layers=2, heads=2, vocab=300)
    state = clip_ref.random_text_state(cfg, seed=3)
    clip_ref.write_text_encoder(str(tmp_path), state, cfg, prefix=prefix, fmt=fmt, dtype=dtype)
    got_cfg, got = load_text_encoder(str(tmp_path))
    assert got_cfg["hidden_size"] == 128 and got_cfg["num_hidden_layers"] == 2
    assert sorted(got) == sorted(state) and not any("position_ids" in k for k in got)
    for k, v in state.items():
        assert got[k].dtype == torch.float16 and torch.equal(got[k].float(), v), k


def test_loader_rejects_bad_checkpoints(tmp_path):
    from coma_amd.sd.weights import load_text_encoder
    cfg = clip_ref.small_config(layers=2, heads=2, vocab=300)
    state = clip_ref.random_text_state(cfg, seed=3)
    missing = dict(state)
    del missing["encoder.layers.1.mlp.fc2.bias"]
    wrong = dict(state)
    wrong["encoder.layers.0.self_attn.q_proj.weight"] = torch.zeros(128, 64)
    for name, st, c in (("missing", missing, cfg), ("wrong", wrong, cfg),
                        ("gelu", state, dict(cfg, hidden_act="gelu")),
                        ("head128", state, dict(cfg, num_attention_heads=1, hidden_size=128)),     # one head of 128
                        ("pos", state, dict(cfg, max_position_embeddings=129)),
                        ("arch", state, dict(cfg, architectures=["T5EncoderModel"]))):
        d = tmp_path / name
        clip_ref.write_text_encoder(str(d), st, cfg)
        (d / "config.json").write_text(json.dumps(c))
        with pytest.raises(ValueError):
            load_text_encoder(str(d))
    from coma_amd.sd.weights import check_text_config
    with pytest.raises(ValueError, match="head dim"):
        check_text_config(dict(clip_ref.small_config(), hidden_size=1024, num_attention_heads=12))
    assert check_text_config({})["hidden_size"] == 768          # the SD-1.x defaults


def test_text_entry_points_validate_before_launch(hip_lib):
    """COMA_E_INVALID (-1) and an error text, nothing launched: null pointers, L > 128, d != 64, QUICK_GELU with GEGLU / SiLU."""
    from coma_amd.sd import ops
    one = C.c_void_p(256)              # never dereferenced: validation fails first
    att = hip_lib.sd_attention_causal_f16
    assert att(None, one, one, one, 1, 12, 77, 64, 2304, 2304, 2304, 768, 0.125, None) == -1
    assert b"null pointer" in hip_lib.coma_last_error()
    assert att(one, one, one, one, 1, 12, 129, 64, 2304, 2304, 2304, 768, 0.125, None) == -1
    assert b"sequence length" in hip_lib.coma_last_error()
    assert att(one, one, one, one, 1, 12, 0, 64, 2304, 2304, 2304, 768, 0.125, None) == -1
    assert att(one, one, one, one, 1, 12, 77, 80, 2304, 2304, 2304, 768, 0.125, None) == -1
    assert b"head dim" in hip_lib.coma_last_error()
    assert att(one, one, one, one, 1, 12, 77, 64, 700, 2304, 2304, 768, 0.125, None) == -1            # ldq < heads * d
    emb = hip_lib.sd_text_embed_f16
    assert emb(None, 1, 77, one, 100, one, 77, 768, one, None) == -1
    assert b"null pointer" in hip_lib.coma_last_error()
    assert emb(one, 1, 78, one, 100, one, 77, 768, one, None) == -1                                  # more positions than the table
    assert emb(one, 1, 77, one, 100, one, 77, 100, one, None) == -1                                  # width % 8
    assert hip_lib.sd_text_encode(None, one, one, None) == -1
    for bad in (ops.EPI_QUICK_GELU | ops.EPI_GEGLU, ops.EPI_QUICK_GELU | ops.EPI_SILU):
        d = ops.ConvGemmDesc()
        d.a0 = d.w = d.out = one
        d.c0, d.batch, d.in_h, d.in_w, d.out_h, d.out_w, d.taps, d.stride, d.n, d.epi = 768, 77, 1, 1, 1, 1, 1, 1, 3072, bad
        assert hip_lib.sd_conv_gemm_f16(C.byref(d), None) == -1
        assert b"QUICK_GELU" in hip_lib.coma_last_error()


def test_text_model_rejects_bad_ids_on_the_host():
    """Ids out of [0, vocab), a wrong length or dtype never reach the device (checked before anything is launched)."""
    from coma_amd.sd.text import HipCLIPTextModel
    m = HipCLIPTextModel.__new__(HipCLIPTextModel)
    m.seq_len, m.vocab = 77, 300
    ok = torch.zeros(2, 77, dtype=torch.int64)
    assert m._check_ids(ok) is not None and m._check_ids(ok.int()) is not None
    for bad, exc in ((torch.full((2, 77), 300), ValueError), (torch.full((1, 77), -1), ValueError), (torch.zeros(2, 76, dtype=torch.int64), ValueError),
                     (torch.zeros(2, 77), TypeError)):
        with pytest.raises(exc):
            m._check_ids(bad)
