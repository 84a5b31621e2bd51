"""One CLIP-guided sampling step through cgd.prepare_run with a community checkpoint selected by '+model=': the comics-faces / pixel-art entry
of COMMUNITY_LOOKUP (classic architecture: conv down / upsampling, additive timestep embeddings, one attention head) scaled down by
monkey-patched flags to a 64 x 64 frame, synthetic weights, ViT-B/32, 4 cutouts.  The step is finite, has the right shapes, ran on a net of
the classic architecture, and two runs with equal seeds are bit-identical.  What the step computes is graded where its pieces are tested
(tests/test_gpu_classic_unet.py for the net, the sampler's and the guidance's own files)."""
import pytest
import torch as th

pytestmark = pytest.mark.gpu

NAME = "pixel_art_diffusion_hard_256.pt"
SMALL = dict(image_size=64, num_channels=64, num_res_blocks=1, channel_mult=(1, 2), attention_resolutions="32")


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("classic_step")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
        mp.chdir(tmp)
        from cgd import cgd as entry
        from cgd import model_flags, script_util
        mp.setitem(model_flags.COMMUNITY_LOOKUP, NAME, {"filename": NAME, "model_flags": dict(model_flags.COMMUNITY_LOOKUP[NAME]["model_flags"], **SMALL)})
        script_util.load_community_model.cache_clear()
        out = []
        for k in range(2):
            run = entry.prepare_run(prompts=["Loose seal."], image_size=64, batch_size=1, num_cutouts=4, class_cond=False, randomize_class=False,
                                    timestep_respacing=f"ddim8+model=some/dir/{NAME}", seed=11, clip_model_name="ViT-B/32",
                                    prefix_path=str(tmp / f"out{k}"), checkpoints_dir=str(tmp / "ckpt"), save_frequency=1, progress=False, device="cuda")
            it = run.samples()
            first = next(it)
            it.close()
            th.cuda.synchronize()
            out.append((run, {k2: first[k2].detach().clone() for k2 in ("sample", "pred_xstart")}))
        script_util.load_community_model.cache_clear()
    return out


def test_the_step_ran_on_the_classic_net(steps):
    run, out = steps[0]
    cfg = run.model.cfg
    assert (cfg.classic_resample, cfg.additive_emb, cfg.num_heads, cfg.model_channels, cfg.image_size) == (1, 1, 1, 64, 64)
    names = [n for n, _ in run.model.param_specs()]
    assert "input_blocks.2.0.op.weight" in names and any(n.endswith(".conv.weight") for n in names)
    assert run.model.num_classes is None
    for key in ("sample", "pred_xstart"):
        assert tuple(out[key].shape) == (1, 3, 64, 64) and bool(th.isfinite(out[key]).all().item()), key
    assert float(out["sample"].abs().max()) > 0.1 and float((out["sample"] - out["pred_xstart"]).abs().max()) > 1e-3


def test_two_runs_with_equal_seeds_are_bit_identical(steps):
    (_, a), (_, b) = steps
    for key in ("sample", "pred_xstart"):
        assert th.equal(a[key].view(th.int32), b[key].view(th.int32)), key
