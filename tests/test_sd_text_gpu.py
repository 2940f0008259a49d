"""GPU: the CLIP text tower on MI355X -- token + position embedding (sd_text_embed_f16), causal attention (sd_attention_causal_f16), the
SD_EPI_QUICK_GELU epilogue of sd_conv_gemm_f16, the whole recorded tower (coma_amd/sd/text.py) against the fp32 restatement of
tests/clip_ref.py (itself pinned to transformers on the CPU) and, when it imports, transformers' CLIPTextModel, save / load / the C ABI,
and the pipeline's choice of the device tower when transformers cannot be imported."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import clip_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_embedding_kernel_is_torch_fp16_and_clamps(hip_lib):
    from coma_amd.sd import ops
    g = torch.Generator().manual_seed(0)
    S, L, V, W = 3, 77, 300, 768
    tok = torch.randn(V, W, generator=g).half().to(DEV)
    pos = torch.randn(80, W, generator=g).half().to(DEV)
    ids = torch.randint(0, V, (S, L), generator=g, dtype=torch.int32).to(DEV)
    out = torch.empty(S * L, W, dtype=torch.float16, device=DEV)
    ops.text_embed(ids, tok, pos, out, seqs=S, len_=L, vocab=V, n_pos=80, width=W)
    want = (tok[ids.long()] + pos[:L]).reshape(S * L, W)
    assert torch.equal(out, want)
    # the kernel clamps: an id below 0 reads row 0, one past the table its last row (the host refuses such ids before they get here)
    bad = ids.clone()
    bad[0, 3], bad[2, 70] = -5, V + 7
    ops.text_embed(bad, tok, pos, out, seqs=S, len_=L, vocab=V, n_pos=80, width=W)
    torch.cuda.synchronize()
    assert torch.equal(out[3], tok[0] + pos[3]) and torch.equal(out[2 * L + 70], tok[V - 1] + pos[70])


@pytest.mark.parametrize("L", [1, 7, 77, 128])
def test_causal_attention_against_sdpa(hip_lib, L):
    from coma_amd.sd import ops
    S, H, d = 3, 12, 64
    C = H * d
    g = torch.Generator().manual_seed(L)
    qkv = torch.randn(S * L, 3 * C, generator=g)
    qkv[:, :2 * C] *= 2.5                                    # q and k scaled up: a sharp softmax
    qkv = qkv.half().to(DEV)

    def run(src):
        f = src.view(-1)
        out = torch.full((S * L, C), float("nan"), dtype=torch.float16, device=DEV)
        ops.attention_causal(f[0:], f[C:], f[2 * C:], out, seqs=S, heads=H, len_=L, d=d, ldq=3 * C, ldk=3 * C, ldv=3 * C, ldo=C, scale=d ** -0.5)
        torch.cuda.synchronize()
        return out

    got = run(qkv)
    q, k, v = (qkv[:, i * C:(i + 1) * C].float().view(S, L, H, d).transpose(1, 2) for i in range(3))
    want = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(S * L, C)
    err = float((got.float() - want).abs().max())
    assert err <= 2e-3 + 1e-3 * float(want.abs().max()), err
    # causality: keys, values (and queries) after position i change -> outputs at positions <= i are bit-identical
    i = L // 2
    alt = qkv.clone().view(S, L, 3 * C)
    alt[:, i + 1:] = torch.randn(S, L - i - 1, 3 * C, generator=g).half().to(DEV) * 4
    got2 = run(alt.view(S * L, 3 * C)).view(S, L, C)
    assert torch.equal(got2[:, :i + 1], got.view(S, L, C)[:, :i + 1])
    if L > 1:
        assert not torch.equal(got2[:, i + 1:], got.view(S, L, C)[:, i + 1:])


@pytest.mark.parametrize("M", [77, 1232])
def test_quick_gelu_epilogue(hip_lib, M):
    from coma_amd.sd import ops
    g = torch.Generator().manual_seed(M)
    K, N = 768, 3072
    x = torch.randn(M, K, generator=g).half().to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5 * 2).half().to(DEV)
    b = (0.5 * torch.randn(N, generator=g)).half().to(DEV)
    out = torch.empty(M, N, dtype=torch.float16, device=DEV)
    ops.linear(x, w, out, rows=M, k=K, n=N, bias=b, epi=ops.EPI_QUICK_GELU)
    torch.cuda.synchronize()
    a = x.float() @ w.float().T + b.float()
    want = a * torch.sigmoid(1.702 * a)
    err = (out.float() - want).abs()
    assert float((err - (2.0 ** -10 * want.abs() + 2e-4)).max()) <= 0, float(err.max())


def _sd15_ids(S=4, L=77, seed=0):
    """BOS, 3..40 word ids, EOS, EOS padding (SD-1.5 tokenizer ids: BOS 49406, EOS 49407)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((S, L), 49407, dtype=torch.int64)
    for s in range(S):
        n = int(torch.randint(3, 41, (1,), generator=g))
        ids[s, 0] = 49406
        ids[s, 1:1 + n] = torch.randint(0, 49406, (n,), generator=g)
    return ids


@pytest.fixture(scope="module")
def sd15_tower(hip_lib):
    from coma_amd.sd.text import HipCLIPTextModel
    from coma_amd.sd.weights import TEXT_CFG
    cfg = dict(TEXT_CFG)
    state = clip_ref.random_text_state(cfg, seed=11, qk_gain=3.0)
    enc = HipCLIPTextModel(state, cfg, capacity=4, device=DEV)
    yield cfg, state, enc
    enc.g.model.close()


def test_tower_against_restatement_at_sd15_size(sd15_tower):
    cfg, state, enc = sd15_tower
    assert enc.num_launches == 2 + 7 * 12
    ids = _sd15_ids()
    got = enc(ids)[0]
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float16 and got.shape == (4, 77, 768)
    ref32 = clip_ref.clip_text_ref(state, cfg, ids.to(DEV), torch.float32)
    ref16 = clip_ref.clip_text_ref(state, cfg, ids.to(DEV), torch.float16).float()
    dev_err, f16_err = (got.float() - ref32).abs(), (ref16 - ref32).abs()
    print(f"text tower vs fp32 restatement: max {float(dev_err.max()):.3e} mean {float(dev_err.mean()):.3e}; "
          f"torch fp16 restatement: max {float(f16_err.max()):.3e} mean {float(f16_err.mean()):.3e}")
    assert float(dev_err.max()) <= 2 * float(f16_err.max()) + 2e-3
    assert float(dev_err.mean()) <= 2 * float(f16_err.mean()) + 2e-4
    # a prompt alone, and among others (padding rows / chunks beyond the capacity of 4): bit-identical rows
    alone = enc(ids[2:3])[0]
    assert torch.equal(alone[0], got[2])
    six = enc(torch.cat([ids, ids[:2]]).int().to(DEV))[0]                    # int32 on the device, two chunks
    assert torch.equal(six[:4], got) and torch.equal(six[4:], got[:2])
    # two successive calls do not alias
    a = enc(ids[:2])[0]
    a_copy = a.clone()
    b = enc(ids[2:])[0]
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, a_copy) and not torch.equal(a, b)


def test_tower_against_transformers(sd15_tower):
    transformers = pytest.importorskip("transformers")
    cfg, state, enc = sd15_tower
    tcfg = transformers.CLIPTextConfig(vocab_size=cfg["vocab_size"], hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                                       num_attention_heads=12, max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5)
    with torch.device(DEV):
        model = transformers.CLIPTextModel(tcfg).half().eval()
    prefix = "text_model." if any(k.startswith("text_model.") for k in model.state_dict()) else ""      # transformers 5: no prefix
    missing, unexpected = model.load_state_dict({prefix + k: v.half() for k, v in state.items()}, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing)
    ids = _sd15_ids(seed=5)
    with torch.no_grad():
        want = model(input_ids=ids.to(DEV)).last_hidden_state.float()
    ref32 = clip_ref.clip_text_ref(state, cfg, ids.to(DEV), torch.float32)
    got = enc(ids)[0].float()
    dev_err, tf_err = (got - ref32).abs(), (want - ref32).abs()
    print(f"text tower vs fp32: max {float(dev_err.max()):.3e}; transformers fp16 vs fp32: max {float(tf_err.max()):.3e}")
    assert float(dev_err.max()) <= 2 * float(tf_err.max()) + 2e-3
    assert float(dev_err.mean()) <= 2 * float(tf_err.mean()) + 2e-4
    del model
    torch.cuda.empty_cache()


def test_save_load_and_c_runner(tmp_path, hip_lib):
    from coma_amd.sd.model import SdModel
    from coma_amd.sd.text import HipCLIPTextModel
    cfg = clip_ref.small_config(layers=2, heads=2, vocab=300)
    state = clip_ref.random_text_state(cfg, seed=2)
    enc = HipCLIPTextModel(state, cfg, capacity=3, device=DEV)
    ids = torch.randint(0, 300, (3, 77), generator=torch.Generator().manual_seed(4))
    want = enc(ids)[0]
    ref = clip_ref.clip_text_ref(state, cfg, ids.to(DEV))
    ref16 = clip_ref.clip_text_ref(state, cfg, ids.to(DEV), torch.float16).float()
    assert float((want.float() - ref).abs().max()) <= 2 * float((ref16 - ref).abs().max()) + 2e-3
    path = tmp_path / "text.sdm"
    enc.save(path)
    assert path.stat().st_size < (8 << 20)
    m = SdModel.load(path, DEV)
    assert m.num_launches("text") == 2 + 7 * 2
    ids_d = ids.int().to(DEV).contiguous()
    out = torch.empty(3, 77, 128, dtype=torch.float16, device=DEV)
    m.text_encode(ids_d, out)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    m.close()
    # a caller without Python
    exe = tmp_path / "run_text"
    libdir = os.path.join(ROOT, "coma_amd")
    subprocess.run(["gcc", os.path.join(ROOT, "tests", "c", "run_text.c"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", "-L" + libdir, "-lcoma_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True, capture_output=True, text=True)
    (tmp_path / "ids.bin").write_bytes(ids.int().numpy().tobytes())
    r = subprocess.run([str(exe), str(path), str(tmp_path / "ids.bin"), str(tmp_path / "emb.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = torch.frombuffer(bytearray((tmp_path / "emb.bin").read_bytes()), dtype=torch.float16).view(3, 77, 128)
    assert torch.equal(got, want.cpu())
    enc.g.model.close()


def test_pipeline_picks_the_device_tower_without_transformers(tmp_path, hip_lib, monkeypatch):
    from safetensors.torch import save_file
    from coma_amd.sd import weights
    from coma_amd.sd.pipeline import AdaptiveMaskInpaintPipeline
    from coma_amd.sd.text import HipCLIPTextModel
    from coma_amd.sd.tokenizer import CLIPTokenizer
    # UNet / VAE: diffusers-layout files with cheap constant tensors (their numerics are covered by test_sd_pipeline_gpu.py); this test
    # is about the text path
    for sub, shapes in (("unet", weights.unet_shapes()), ("vae", weights.vae_shapes())):
        (tmp_path / sub).mkdir()
        st = {k: torch.full(shp, 1.0 if (k.endswith("weight") and len(shp) == 1) else (0.01 if k.endswith("weight") else 0.0),
                            dtype=torch.float16) for k, shp in shapes.items()}
        save_file(st, str(tmp_path / sub / "diffusion_pytorch_model.safetensors"))
    vocab, _ = clip_ref.learn_tokenizer(str(tmp_path / "tokenizer"))
    cfg = clip_ref.small_config(layers=2, heads=12, vocab=len(vocab))          # hidden 768: the UNet's context width
    clip_ref.write_text_encoder(str(tmp_path / "text_encoder"), clip_ref.random_text_state(cfg, seed=7), cfg)
    monkeypatch.setitem(sys.modules, "transformers", None)                     # `from transformers import ...` raises ImportError
    pipe = AdaptiveMaskInpaintPipeline.from_pretrained(str(tmp_path), batch_size=1, device=DEV)
    assert isinstance(pipe.text_encoder, HipCLIPTextModel) and isinstance(pipe.tokenizer, CLIPTokenizer)
    prompt = "a person sitting on a chair"
    emb = pipe._encode_prompt(prompt, clip_ref.NEGATIVE_PROMPT, None, None, 1)
    tower = lambda p: pipe.text_encoder(pipe.tokenizer([p], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids)[0]
    assert emb.shape == (2, 77, 768) and torch.equal(emb, torch.cat([tower(clip_ref.NEGATIVE_PROMPT), tower(prompt)]))
    assert not torch.equal(emb[0], emb[1])
    g = torch.Generator().manual_seed(5)
    image = torch.rand(1, 3, 512, 512, generator=g) * 2 - 1
    mask = torch.zeros(1, 1, 512, 512)
    mask[:, :, 100:400, 150:380] = 1
    out = pipe(prompt=prompt, negative_prompt=clip_ref.NEGATIVE_PROMPT, image=image, default_mask_image=mask, num_inference_steps=2,
               guidance_scale=7.5, generator=torch.Generator(device=DEV).manual_seed(3), output_type="u8", use_adaptive_mask=False).images
    assert out.shape == (1, 512, 512, 3) and out.dtype == torch.uint8
    del pipe
    torch.cuda.empty_cache()
