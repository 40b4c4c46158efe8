"""The host side of the FID (reface_amd/fidscore.py, eval_tool/fid/fid_score.py) against the reference's own outputs on the seeded folders of
tests/fid_inputs.py (tests/golden/fid.npz, written by tools/gen_golden.py::gen_fid from the reference's InceptionV3.forward,
ImagePathDataset, get_activations, calculate_activation_statistics and calculate_frechet_distance).  No GPU."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fid_inputs as I  # noqa: E402

from reface_amd import fidscore as FS  # noqa: E402
from reface_amd.params import CLIPVisionConfig, fid_clip_param_specs  # noqa: E402


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "fid.npz"))


@pytest.fixture(scope="module")
def data():
    return I.build()


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def test_resize_and_crop_rules():
    """torchvision's Resize(224) sizes and CenterCrop(224) offsets for the sizes of the fixture, written out."""
    assert FS.resized_size(512, 512) == (224, 224) and FS.resized_size(224, 224) == (224, 224) and FS.resized_size(1, 1) == (224, 224)
    assert FS.resized_size(300, 260) == (258, 224) and FS.resized_size(260, 300) == (224, 258) and FS.resized_size(57, 40) == (319, 224)
    assert FS.resized_size(224, 225) == (224, 225) and FS.resized_size(224, 227) == (224, 227) and FS.resized_size(1024, 1024) == (224, 224)
    assert [FS.crop_offset(n) for n in (224, 225, 227, 258, 319)] == [0, 0, 2, 17, 48]          # 0.5 -> 0 and 1.5 -> 2: half to even
    b, k = FS.crop_taps(1024, 224)
    assert b.shape == (224, 2) and k.shape == (224, 21)
    b, k = FS.crop_taps(227, 227)
    assert b[:, 0].tolist() == list(range(2, 226)) and k.shape == (224, 1)          # the identity table, sliced to the crop


def test_prep_host_vs_reference_bits(golden, data):
    """prep_host on the three stored inputs (512 x 512 RGB, the L image, the all-255 RGBA image) equals the reference run's prepared tensors
    bit for bit; so does prep_host of the RGB bytes the device path takes for them (L replicated, alpha dropped)."""
    assert golden["prep_index"].tolist() == list(I.PREP_SAMPLES)
    modes = []
    for j, i in enumerate(I.PREP_SAMPLES):
        im = data["dataset"][i]
        modes.append(im.shape[2:] or (1,))
        for src in (im, I.rgb(im)):
            got = FS.prep_host(src)
            assert got.shape == (3, 224, 224) and got.dtype == np.float32
            bad = int((got.view(np.uint32) != golden["prep"][j].view(np.uint32)).sum())
            print(f"fid prep_host image {i} {im.shape}: {bad} values differ from the reference's prepared tensor in any bit")
            assert bad == 0
    assert modes == [(3,), (1,), (4,)]


def test_decode_item_modes(data):
    """RGB, L and all-255 RGBA go to the device as bytes whose host preparation equals that of the image itself; P, LA and an RGBA image with
    one transparent pixel are prepared on the host."""
    from PIL import Image
    for i in (1, I.L_AT, I.RGBA_AT):
        im = Image.fromarray(data["results"][i])
        kind, t = FS.decode_item(im)
        assert kind == "u8" and t.dtype == torch.uint8 and t.shape == im.size[::-1] + (3,)
        assert np.array_equal(FS.prep_host(t.numpy()), FS.prep_host(im)), im.mode
    rgba = data["results"][I.RGBA_AT].copy()
    rgba[3, 4, 3] = 254
    for im in (Image.fromarray(data["results"][1]).convert("P"), Image.fromarray(data["results"][1]).convert("LA"), Image.fromarray(rgba)):
        kind, t = FS.decode_item(im)
        assert kind == "host" and t.dtype == torch.float32 and tuple(t.shape) == (3, 224, 224)
        assert np.array_equal(t.numpy(), FS.prep_host(im))


def test_stats_and_frechet_vs_reference(golden):
    """The reference's fp32 features through stats_host and frechet_distance: mu, sigma and the FID to 1e-12 relative (the same numpy and
    scipy calls)."""
    m1, s1 = FS.stats_host(golden["feat_f32_dataset"])
    m2, s2 = FS.stats_host(golden["feat_f32_results"])
    assert m1.dtype == s1.dtype == np.float64 and s1.shape == (32, 32)
    figs = [_rel(m1, golden["mu_dataset"]), _rel(s1, golden["sigma_dataset"]), _rel(m2, golden["mu_results"]), _rel(s2, golden["sigma_results"])]
    fid = FS.frechet_distance(m1, s1, m2, s2)
    d2, t1, t2, tc = FS.frechet_terms(m1, s1, m2, s2)
    print(f"fid host: rel |mu, sigma - reference| = {max(figs):.3e}; FID {fid:.9f} vs reference {float(golden['fid']):.9f}")
    assert max(figs) <= 1e-12
    assert abs(fid - float(golden["fid"])) <= 1e-12 * float(golden["fid"])
    assert fid == d2 + t1 + t2 - 2 * tc and float(golden["fid"]) > 100 * float(golden["fid_tol_f32"]) > 0


def test_frechet_eps_retry_and_imaginary_check(capsys):
    """A product whose square root is not finite takes the reference's eps retry and prints its line; a large imaginary diagonal raises."""
    from scipy import linalg
    mu = np.zeros(2)
    real_sqrtm = linalg.sqrtm
    calls = []

    def fake(a, disp=True):
        calls.append(disp)
        if len(calls) == 1:
            return np.full_like(a, np.nan), 0.0
        return real_sqrtm(a)

    linalg.sqrtm = fake
    try:
        v = FS.frechet_distance(mu, np.eye(2), mu, np.eye(2))
    finally:
        linalg.sqrtm = real_sqrtm
    assert calls == [False, True] and "fid calculation produces singular product; adding 1e-06 to diagonal of cov estimates" in capsys.readouterr().out
    assert abs(v - (4 - 2 * 2 * (1 + 1e-6))) < 1e-12
    linalg.sqrtm = lambda a, disp=True: (np.eye(2) * (1 + 0.5j), 0.0)
    try:
        with pytest.raises(ValueError, match="Imaginary component"):
            FS.frechet_distance(mu, np.eye(2), mu, np.eye(2))
    finally:
        linalg.sqrtm = real_sqrtm


def _openai_named(sd, cfg):
    """The seeded HF-named tower in OpenAI ``clip`` naming, with a few text-tower keys beside it."""
    v = "vision_model."
    out = {"visual.conv1.weight": sd[v + "embeddings.patch_embedding.weight"], "visual.class_embedding": sd[v + "embeddings.class_embedding"],
           "visual.positional_embedding": sd[v + "embeddings.position_embedding.weight"], "visual.proj": sd["visual_projection.weight"].t().contiguous(),
           "positional_embedding": torch.zeros(77, 16), "text_projection": torch.zeros(16, 32), "logit_scale": torch.zeros(()),
           "transformer.resblocks.0.attn.in_proj_weight": torch.zeros(48, 16), "token_embedding.weight": torch.zeros(10, 16), "ln_final.weight": torch.zeros(16)}
    for a, b in (("ln_pre", "pre_layrnorm"), ("ln_post", "post_layernorm")):
        for leaf in ("weight", "bias"):
            out[f"visual.{a}.{leaf}"] = sd[f"{v}{b}.{leaf}"]
    for i in range(cfg.layers):
        p, q = f"{v}encoder.layers.{i}.", f"visual.transformer.resblocks.{i}."
        for leaf in ("weight", "bias"):
            out[f"{q}attn.in_proj_{leaf}"] = torch.cat([sd[f"{p}self_attn.{n}.{leaf}"] for n in ("q_proj", "k_proj", "v_proj")], 0)
            for a, b in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"), ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
                out[f"{q}{a}.{leaf}"] = sd[f"{p}{b}.{leaf}"]
    return out


def test_openai_key_map_is_exact_and_strict():
    sd = FS.seeded_fid_state()
    cfg = CLIPVisionConfig(**FS.FIXTURE_TOWER)
    oa = _openai_named(sd, cfg)
    back, got_cfg = FS.check_fid_state(oa)
    assert list(back) == list(fid_clip_param_specs(cfg)) == list(sd)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    assert (got_cfg.hidden, got_cfg.layers, got_cfg.heads, got_cfg.intermediate, got_cfg.patch, got_cfg.image, got_cfg.proj) == (128, 2, 2, 512, 32, 224, 32)
    half, _ = FS.check_fid_state({k: v.half() for k, v in oa.items()})          # the cached archive holds fp16 weights
    assert all(t.dtype == torch.float32 for t in half.values())
    hf_named, _ = FS.check_fid_state(dict(sd, **{"text_model.embeddings.token_embedding.weight": torch.zeros(3, 3), "logit_scale": torch.zeros(()),
                                                 "vision_model.embeddings.position_ids": torch.arange(50)[None]}))
    assert all(torch.equal(hf_named[k], sd[k]) for k in sd)
    for gone in ("visual.transformer.resblocks.1.mlp.c_proj.bias", "visual.ln_post.weight", "visual.proj", "visual.conv1.weight"):
        with pytest.raises(RuntimeError):
            FS.check_fid_state({k: v for k, v in oa.items() if k != gone})
    with pytest.raises(RuntimeError, match="visual.proj"):
        FS.check_fid_state(dict(oa, **{"visual.proj": oa["visual.proj"].t().contiguous()}))
    with pytest.raises(RuntimeError):
        FS.check_fid_state(dict(oa, **{"visual.transformer.resblocks.0.mlp.c_fc.weight": torch.zeros(512, 64)}))
    with pytest.raises(RuntimeError, match="unexpected vision key"):
        FS.check_fid_state(dict(oa, **{"visual.extra.weight": torch.zeros(3)}))
    b32 = fid_clip_param_specs(CLIPVisionConfig(**FS.VIT_B32))
    assert b32["vision_model.embeddings.patch_embedding.weight"] == (768, 3, 32, 32) and b32["visual_projection.weight"] == (512, 768)
    assert b32["vision_model.embeddings.position_embedding.weight"] == (50, 768) and "vision_model.encoder.layers.11.mlp.fc2.bias" in b32
    assert not any(k.startswith("mapper") or k.startswith("final_ln") for k in b32)


def test_file_listing_and_batch_warning(tmp_path, capsys):
    """glob('*.ext') per extension of the folder itself, sorted as paths: no sub-folders, no other extensions, case-sensitive; a batch
    larger than the folder becomes the folder with the reference's line."""
    for name in ("b.png", "a.jpg", "10.png", "9.png", "c.txt", "D.PNG", "e.webp", "f.jpeg.bak"):
        (tmp_path / name).write_bytes(b"")
    (tmp_path / "sub").mkdir()
    (tmp_path / "sub" / "z.png").write_bytes(b"")
    assert [os.path.basename(f) for f in FS.list_images(str(tmp_path))] == ["10.png", "9.png", "a.jpg", "b.png", "e.webp"]
    assert FS.effective_batch(50, 48) == 48
    assert capsys.readouterr().out == "Warning: batch size is bigger than the data size. Setting batch size to data size\n"
    assert FS.effective_batch(48, 48) == 48 and FS.effective_batch(4, 48) == 4 and capsys.readouterr().out == ""


def _cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("reface_fid_cli", os.path.join(ROOT, "eval_tool", "fid", "fid_score.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cli_parser_accepts_the_reference_command_line():
    """evaluate_all.sh: ``fid_score.py --device cuda <dataset> <results>``; and every option of the reference's parser."""
    p = _cli().build_parser()
    a = p.parse_args(["--device", "cuda", "dataset/FaceData/CelebAMask-HQ/CelebA-HQ-img", "results/test_bench/results"])
    assert a.device == "cuda" and a.path == ["dataset/FaceData/CelebAMask-HQ/CelebA-HQ-img", "results/test_bench/results"]
    assert a.batch_size == 50 and a.num_workers is None and a.dims == 2048 and a.precision == "full"
    a = p.parse_args(["--batch-size", "8", "--num-workers", "2", "--dims", "768", "--device", "cuda:1", "stats.npz", "res"])
    assert (a.batch_size, a.num_workers, a.dims, a.device, a.path) == (8, 2, 768, "cuda:1", ["stats.npz", "res"])
    with pytest.raises(SystemExit):
        p.parse_args(["--dims", "512", "a", "b"])


def test_npz_round_trip_through_save_stats(tmp_path, golden, capsys, monkeypatch):
    """The CLI's --save-stats file as a first path gives the FID of the folder it was saved from, to 1e-12 relative.  The folders' features
    are the fixture's (a scorer whose per-folder statistics are stats_host of them: no GPU here); the .npz branch, the Frechet step, the
    printed line and --json are the CLI's own."""
    feats = {"dataset": golden["feat_f32_dataset"], "results": golden["feat_f32_results"]}
    real = FS.FidScorer

    class HostScorer(real):
        def __init__(self, state_dict, precision="full", batch=50, device="cuda"):
            self.batch = batch

        def _warm(self, paths):
            pass

        def features_folder(self, folder, num_workers=0):
            raise AssertionError("no GPU in this test")

        def statistics_of_path(self, path, num_workers=0):
            if str(path).endswith(".npz"):
                return real.statistics_of_path(self, path, num_workers)
            f = feats[os.path.basename(path)]
            return FS.stats_host(f) + (len(f), 0)

    monkeypatch.setattr(FS, "FidScorer", HostScorer)
    cli = _cli()
    for n in feats:
        (tmp_path / n).mkdir()
    stats, js = str(tmp_path / "dataset_stats.npz"), str(tmp_path / "fid.json")
    r1 = cli.main(["--device", "cuda", str(tmp_path / "dataset"), str(tmp_path / "results"), "--clip_ckpt", "none", "--save-stats", stats, "--json", js])
    line = capsys.readouterr().out.splitlines()[-1]
    assert line == "FID:  {}".format(r1["fid"])          # print('FID: ', v): two spaces
    j = json.load(open(js))
    assert j["fid"] == r1["fid"] == float(line.split()[1]) and j["images"] == 96 and j["host_prepared"] == 0
    assert j["fid"] == j["mean_term"] + j["trace1"] + j["trace2"] - 2 * j["trace_covmean"]
    assert abs(r1["fid"] - float(golden["fid"])) <= 1e-12 * float(golden["fid"])
    with np.load(stats) as f:
        assert sorted(f.files) == ["mu", "sigma"] and np.array_equal(f["mu"], golden["mu_dataset"]) and np.array_equal(f["sigma"], golden["sigma_dataset"])
    r2 = cli.main(["--device", "cuda", stats, str(tmp_path / "results"), "--clip_ckpt", "none"])
    print(f"fid .npz round trip: {r2['fid']!r} from the statistics file, {r1['fid']!r} from the folder")
    assert abs(r2["fid"] - r1["fid"]) <= 1e-12 * r1["fid"] and r2["images1"] == 0 and r2["images2"] == 48
