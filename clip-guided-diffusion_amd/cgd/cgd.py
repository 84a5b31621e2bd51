"""Drop-in entry point: `cgd.cgd.clip_guided_diffusion(...)` generator and the `cgd` CLI (`cgd.cgd:main`).

Mirrors the public surface of /root/reference/cgd/cgd.py — keyword arguments and defaults of
`clip_guided_diffusion` (:19-55), the yielded `(batch_idx, png_path)` tuples (:266-270), the CLI flags and aliases
of `main` (:286-358) — while every per-timestep computation runs through the MI355X C ABI
(UNet / CLIP tower handles, `ClipGuidance` cond_fn, `GuidedSampler` loops).
"""
import argparse
import functools
import glob
from pathlib import Path

import torch as th
from tqdm.auto import tqdm

from cgd_amd import nets, regions, shard
from cgd_amd.guidance import ClipGuidance

from . import clip_util, script_util


class GuidedRun:
    """What `clip_guided_diffusion` builds between its argument checks and its sampling loop (prepare_run): the model, the diffusion, the
    cond_fn, the sampler loop and its arguments, and the output helpers.  The generator runs `frames()` once; cgd_amd.animate builds one and
    runs `samples()` once per animation frame on the same networks and guidance."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def samples(self, init_image=None, skip_timesteps=None, **loop_kw):
        """The sampler loop's iterator over one run, the cond_fn's closure counter set as the reference sets it (cgd.py:265); the caller
        lowers `cond_fn.current_timestep` by one per yielded step.  `init_image` / `skip_timesteps`: instead of the run's own (None)."""
        samples = self.loop(self.model, self.shape, clip_denoised=False, model_kwargs=self.model_kwargs, cond_fn=self.cond_fn,
                            progress=self.progress, skip_timesteps=self.skip_timesteps if skip_timesteps is None else skip_timesteps,
                            init_image=self.init_tensor if init_image is None else init_image, randomize_class=self.randomize_class,
                            cond_fn_with_grad=True, **{**self.loop_kw, **loop_kw})
        self.cond_fn.current_timestep = self.diffusion.num_timesteps - 1
        return samples

    def write(self, arr, name_idx):
        """(local batch, H, W, 3) uint8 -> one PNG per sample, '<prefix>/<prompts>/<batch_idx:02>/<name_idx:04>.png'; yields
        (batch_idx, path), batch_idx the index in the GLOBAL batch."""
        for local_idx, batch_idx in enumerate(self.mine):
            yield batch_idx, script_util.write_image(arr[local_idx], self.prefix_path, self.prompts, name_idx, batch_idx)

    def frames(self):
        """The run: generator of `(batch_idx, png_path)`."""
        cond_fn, wandb_run, progress, save_frequency = self.cond_fn, self.wandb_run, self.progress, self.save_frequency
        try:
            samples = self.samples()

            # Output path (reference cgd.py:180-186,234-238,265-270), software-pipelined by one timestep: the GPU work of timestep
            # k+1 is enqueued BEFORE the host looks at timestep k (loss scalars, uint8 frames), and those reads travel on a side
            # stream (cgd_amd/hostcopy.py).  With the CLI default --save_frequency 1 the two PNG encodes per sample then overlap the
            # next step on the GPU instead of idling it.  Yield order and file naming are unchanged.
            def enqueue_steps():
                for step, sample in enumerate(samples):
                    cond_fn.current_timestep -= 1
                    # a gated --reduce-clip step logs nothing (the reference's cond_fn returns before its logging, cgd.py:155-160)
                    want_log = (progress or wandb_run is not None) and cond_fn.last_ran
                    save = step % save_frequency == 0 or cond_fn.current_timestep == -1
                    yield (step, cond_fn.snapshot() if want_log else None, script_util.stage_images(sample["pred_xstart"]) if save else None)

            def finish(item):
                step, snapshot, frames = item
                if snapshot is not None:
                    log = cond_fn.log(snapshot)
                    if progress:
                        tqdm.write("\t".join(f"{k}: {v:.3f}" for k, v in log.items() if "loss" in k.lower()))
                    if wandb_run is not None:
                        wandb_run.log(log)
                if frames is not None:
                    yield from self.write(frames.get().numpy(), step)

            previous = None
            pending = enqueue_steps()
            while True:
                try:
                    item = next(pending)
                except StopIteration:
                    break
                except (RuntimeError, KeyboardInterrupt):
                    # enqueuing timestep k+1 failed (OOM, ^C): timestep k is complete, so its frames are still written and yielded
                    # first, as the unpipelined reference would have done before starting k+1
                    if previous is not None:
                        item, previous = previous, None
                        yield from finish(item)
                    raise
                if previous is not None:
                    yield from finish(previous)
                previous = item
            if previous is not None:
                yield from finish(previous)
        except (RuntimeError, KeyboardInterrupt) as runtime_ex:
            if "out of memory" in str(runtime_ex).lower():
                # the reference's hint, kept word for word (cgd.py:274-283)
                print("\n".join((
                    "CUDA OOM error occurred.", "Try lowering --image_size/-size, --batch_size/-bs, --num_cutouts/-cutn",
                    f"--clip_model/-clip (currently {self.clip_model_name}) can have a large impact on VRAM usage.",
                    "'RN50' will use the least VRAM. 'ViT-B/32' the second least and is good for its memory/runtime constraints.")))
            else:
                raise runtime_ex


def clip_guided_diffusion(image_size=128, num_cutouts=16, prompts=[], image_prompts=[], clip_guidance_scale=1000, tv_scale=150,
                          range_scale=50, sat_scale=0, init_scale=0, batch_size=1, init_image=None, class_cond=True,
                          cutout_power=1.0, timestep_respacing="1000", seed=0, diffusion_steps=1000, skip_timesteps=0,
                          checkpoints_dir=script_util.CACHE_PATH, clip_model_name="ViT-B/32", randomize_class=True,
                          prefix_path=Path("./outputs"), save_frequency=25, noise_schedule="linear", dropout=0.0, device="",
                          wandb_project=None, wandb_entity=None, use_augs=False, use_magnitude=False, height_offset=0,
                          width_offset=0, progress=True, reduce_clip=False, progressive_cutout=False, cached_cutouts=False):
    """Generator of `(batch_idx, png_path)`; keyword names and defaults are the reference's (cgd.py:19-55)."""
    run = prepare_run(**locals())
    if run is not None:  # (None: a rank of a sharded run that has no sample)
        yield from run.frames()


def prepare_run(image_size=128, num_cutouts=16, prompts=[], image_prompts=[], clip_guidance_scale=1000, tv_scale=150,
                range_scale=50, sat_scale=0, init_scale=0, batch_size=1, init_image=None, class_cond=True,
                cutout_power=1.0, timestep_respacing="1000", seed=0, diffusion_steps=1000, skip_timesteps=0,
                checkpoints_dir=script_util.CACHE_PATH, clip_model_name="ViT-B/32", randomize_class=True,
                prefix_path=Path("./outputs"), save_frequency=25, noise_schedule="linear", dropout=0.0, device="",
                wandb_project=None, wandb_entity=None, use_augs=False, use_magnitude=False, height_offset=0,
                width_offset=0, progress=True, reduce_clip=False, progressive_cutout=False, cached_cutouts=False, lpips_for_later=False):
    """`clip_guided_diffusion`'s arguments -> its GuidedRun (None on a rank of a sharded run that has no sample): every argument check, then
    every load, then the guidance and the sampler loop; nothing is sampled.  `lpips_for_later`: load the LPIPS-VGG16 handle although this
    run's own arguments need none (ClipGuidance.set_init may then switch the init-image term on)."""
    if len(device) == 0:
        device = "cuda" if th.cuda.is_available() else "cpu"
        print(f"device: {device} (picked automatically; --device/-dev overrides)")
    else:
        print(f"device: {device}")
    if "cuda" not in device:
        raise ValueError(f"device {device!r}: this build runs the sampling step on an MI355X only (PyTorch-ROCm reports 'cuda')")
    # "...+model=FILE[:heads=N | :head_channels=N][:new_order]" (an extension like "plmsN", the last suffix of all): a community checkpoint of the
    # classic UNet architecture instead of the published one of image_size; malformed text, a file that is neither known nor given a head count,
    # a class conditioning that disagrees with a known file and "upsample=" next to it are refused before anything is loaded
    timestep_respacing, model_spec = script_util.split_model(timestep_respacing)
    if model_spec is not None:
        script_util.check_model(model_spec, image_size, class_cond, init_image)
    # "...+windows=STRIDE[:wrapx|:wrapy|:wrap][:feather]" (likewise, the last suffix among what remains): windowed sampling, the model runs on
    # overlapping image_size windows of the image_size + offsets frame; a bad stride or frame, or a combination with "upsample=", "invert=" or
    # "+classifier=", is refused before anything is loaded
    timestep_respacing, windows_spec = script_util.split_windows(timestep_respacing, image_size, height_offset, width_offset, init_image,
                                                                 clip_model_name)
    # "dpmN+thr=P[:CAP]" (an extension like "plmsN"): dynamic thresholding of the guided pred_xstart; refused on any other spacing, before
    # anything is loaded.  The tables are built from the spacing without the suffix
    timestep_respacing, threshold = script_util.split_threshold(timestep_respacing)
    # "upsample=IMAGE" (an extension like "invert=IMAGE"): run the super-resolution checkpoint of image_size on IMAGE; refused before
    # anything is loaded at other sizes, without class conditioning, or together with "invert="
    upsample = script_util.check_init_upsample(init_image, image_size, class_cond)
    # "ilvrN=IMAGE" / "ilvrN@U=IMAGE" (likewise): ILVR, sampling conditioned on IMAGE's low frequencies; refused before anything is loaded
    # together with a mask, "invert=" or "upsample=", or when N does not divide both frame sides
    ilvr_spec = script_util.check_init_ilvr(init_image, image_size, height_offset, width_offset)
    if init_image and script_util.split_init_invert(script_util.split_init_mask(init_image)[0])[1]:
        # refused before anything is loaded
        # the inverted latent is a start state of the deterministic loops only ('dpmsdeN' draws a noise per step; tested before 'dpm')
        if str(timestep_respacing).startswith("dpmsde") or not str(timestep_respacing).startswith(("ddim", "plms", "dpm")):
            raise ValueError(f"init image 'invert=...' needs a deterministic sampler: timestep_respacing must start with 'ddim' or 'plms' "
                             f"(or 'dpm', but not 'dpmsde'), got {timestep_respacing!r}")
        if height_offset or width_offset:  # the init image is image_size x image_size, and so is the latent inverted from it
            raise ValueError(f"init image 'invert=...' needs height_offset = width_offset = 0, got {height_offset} and {width_offset}: the "
                             "inverted latent has the init image's size")

    # "TEXT@@REGION[^POWER][:weight]" among the prompts and image prompts (an extension like "plmsN"): a region prompt, which acts on a cutout in
    # proportion to the share of REGION (a mask file or a box "x0,y0,x1,y1") the cutout sees; malformed entries are refused before anything is
    # loaded.  From here on `prompts` and `image_prompts` are the entries without their "@@..." parts
    prompts, prompt_regions = script_util.split_region_prompts(prompts)
    image_prompts, image_regions = script_util.split_region_prompts(image_prompts)
    if use_augs and any(spec is not None for spec, _ in prompt_regions + image_regions):
        raise ValueError("'TEXT@@REGION' prompts do not work with use_augs: the box is warped after the crop")
    # "SOURCE=>TARGET[:weight]" among the prompts (an extension like "plmsN"): a direction prompt, scored by the directional CLIP loss against
    # the init image; refused before anything is loaded when malformed or without an init image
    direction_pairs = script_util.direction_prompts(prompts, image_prompts, init_image, height_offset, width_offset)
    # "style=FILE[:SCALE]" among the image prompts (likewise): the style image of the VGG Gram-matrix style loss, SCALE its weight; no CLIP
    # prompt.  Refused before anything is loaded when malformed, given twice, or at a frame whose sides are no multiples of 16
    image_regions = [r for p, r in zip(image_prompts, image_regions) if not str(p).startswith(script_util.STYLE_PREFIX)]
    image_prompts, style_spec = script_util.split_style_prompts(image_prompts, image_size + height_offset, image_size + width_offset)
    if use_augs and any(pair is not None for pair in direction_pairs):
        raise ValueError("'SOURCE=>TARGET' prompts do not work with use_augs: the random warp of every cut would have to be replayed on the init image")

    # "A+cuts=OV:IN" (an extension like "plmsN"): overview + inner cutouts through the antialiased cubic resize instead of pooled crops
    # "A+classifier=FILE:CLASS[:SCALE]" (likewise): classifier guidance with guided-diffusion's noisy ImageNet classifier
    # "A+aesthetic=FILE:SCALE" (likewise): an aesthetic predictor on the embeddings of the tower entry before it; taken out of the list first
    without_aesthetic, aesthetic_specs = clip_util.split_aesthetic(clip_model_name)  # refuses before any load
    without_classifier, classifier_spec = clip_util.split_classifier(without_aesthetic, height_offset, width_offset)  # refuses before any load
    towers_and_secondary, cuts = clip_util.split_cuts(without_classifier, progressive_cutout, use_augs)  # refuses before any load
    # "A+secondary=FILE" (likewise): the guidance gradient returns through the secondary model instead of through the UNet
    clip_names, secondary_path = clip_util.split_secondary(towers_and_secondary, image_size, height_offset, width_offset)  # refuses before any load
    if any(spec is not None for spec in aesthetic_specs) and len(aesthetic_specs) != len(clip_names):
        raise ValueError(f"{clip_model_name}: an empty entry in the list; 'aesthetic=' entries cannot be bound to its {len(clip_names)} towers")

    wandb_run = None
    if wandb_project is not None:
        import wandb  # optional observability hook, outside the hot path
        wandb_run = wandb.init(project=wandb_project, entity=wandb_entity, config=locals())
    else:
        print("no --wandb_project given: W&B logging is off")

    th.manual_seed(seed)
    if not use_magnitude and image_size == 64:
        use_magnitude = True
        tqdm.write("64x64 checkpoint: gradient-magnitude clamp switched on")
    Path(prefix_path).mkdir(parents=True, exist_ok=True)
    Path(checkpoints_dir).mkdir(parents=True, exist_ok=True)
    if upsample:
        diffusion_path = script_util.download_upsampler(image_size, checkpoints_dir)
    elif model_spec is not None:
        diffusion_path = None  # a local file (as given or under checkpoints_dir): nothing to download
    else:
        diffusion_path = script_util.download_guided_diffusion(image_size=image_size, checkpoints_dir=checkpoints_dir, class_cond=class_cond)

    # CLIP tower(s), prompt embeddings and weights.  "A+B" (e.g. "RN50+ViT-L/14", BASELINE config 5) sums the CLIP losses of
    # several towers: a build extension, the reference takes a single name.
    clip_models, clip_size = [], None
    for name in clip_names:
        cm, size = clip_util.load_clip(name, device)
        clip_models.append(cm)
        clip_size = clip_size or size
    clip_model = clip_models[0]
    embeds_per_tower, weights = [[] for _ in clip_names], []
    region_specs = list(prompt_regions)  # (REGION or None, POWER) per entry of `weights`
    # direction prompts: per tower normalize(E(target caption)) - normalize(E(source caption)); their places in the weight list, which holds
    # targets and directions alike in the order given
    dirs_per_tower, direction_columns = [[] for _ in clip_names], []
    text_cache = {}  # (text, tower name) -> embedding, for GuidedRun
    for prompt, pair in zip(prompts, direction_pairs):
        text, weight = script_util.parse_prompt(prompt)
        for k, name in enumerate(clip_names):
            if pair is not None:
                e_src, _ = clip_util.encode_text_prompt(pair[0], weight, name, device)
                e_tgt, w_k = clip_util.encode_text_prompt(pair[1], weight, name, device)
                dirs_per_tower[k].append(th.nn.functional.normalize(e_tgt.float(), dim=-1) - th.nn.functional.normalize(e_src.float(), dim=-1))
                continue
            embed, w_k = clip_util.encode_text_prompt(text, weight, name, device)
            text_cache[(text, name)] = embed
            embeds_per_tower[k].append(embed)
        if pair is not None:
            direction_columns.append(len(weights))
        weights.append(w_k)
    text_embeds, text_weights = len(embeds_per_tower[0]), len(weights)  # what comes behind belongs to the image prompts
    for image_prompt, region in zip(image_prompts, image_regions):
        img, weight = script_util.parse_prompt(image_prompt)
        for k, name in enumerate(clip_names):
            embed, batched = clip_util.encode_image_prompt(img, weight, image_size, num_cutouts=num_cutouts, clip_model_name=name, device=device)
            embeds_per_tower[k].append(embed)
        weights.extend(batched)
        region_specs.extend([region] * len(batched))  # every embedding of the image gets its region
    # (a run with direction prompts only has no target embeddings: ClipGuidance then makes no spherical launch)
    # (... and a run with a style image and no prompt at all has neither: no cutouts, no CLIP pass)
    # (... and so has a run with an aesthetic head and no prompt: the CLIP pass then runs for the head alone)
    style_only = (style_spec is not None or any(spec is not None for spec in aesthetic_specs)) and not weights
    target_embeds = [th.cat(e) for e in embeds_per_tower] if (embeds_per_tower[0] or not (direction_columns or style_only)) else None
    weight_t = th.tensor(weights, device=device)
    if not style_only:
        if weight_t.sum().abs() < 1e-3:
            raise RuntimeError("The weights must not sum to 0.")
        weight_t = weight_t / weight_t.sum().abs()
    direction_kw = {}
    if direction_columns:  # normalised together above; ClipGuidance builds the B x P matrix over the whole list and splits its columns
        target_columns = [c for c in range(len(weights)) if c not in direction_columns]
        direction_kw = dict(direction_embeds=[th.cat(e) for e in dirs_per_tower], direction_weights=weight_t[direction_columns],
                            direction_columns=direction_columns)
        weight_t = weight_t[target_columns]

    if use_augs:
        tqdm.write("cutout augmentations requested")
    if cuts is not None:  # --num_cutouts then only sizes the image prompts' cutouts above
        make_cutouts = clip_util.MakeCutoutsResized(clip_size, overview=cuts[0], inner=cuts[1], schedule=cuts[2], ctx=clip_model.tower.ctx)
    else:
        make_cutouts = clip_util.MakeCutouts(cut_size=clip_size, num_cutouts=num_cutouts, cutout_size_power=cutout_power, use_augs=use_augs,
                                             ctx=clip_model.tower.ctx)
    if cached_cutouts:
        make_cutouts.cache_coordinates(image_size + width_offset, image_size + height_offset)

    init_tensor, mask_tensor, invert = None, None, False
    if init_image:
        import numpy as np
        from PIL import Image
        # "IMAGE::MASK" (an extension like "plmsN"): masked sampling, the white part of MASK is regenerated and the black part kept
        init_image, mask_image = script_util.split_init_mask(init_image)
        # "invert=IMAGE": start from the image's own DDIM-inverted latent instead of the image plus random noise
        init_image, invert = script_util.split_init_invert(init_image)
        # "upsample=IMAGE": IMAGE at a quarter of the frame conditions the super-resolution model; at the full frame it stays the init image
        init_image, _ = script_util.split_init_upsample(init_image)
        # "ilvrN=IMAGE": IMAGE at the run's frame is the reference of ILVR; it also stays the ordinary init image
        init_image, _ = script_util.split_init_ilvr(init_image)
        source = Image.open(script_util.fetch(init_image)).convert("RGB")
        pil = source.resize((image_size, image_size))
        init_tensor = th.from_numpy(np.array(pil)).float().div(255).permute(2, 0, 1).to(device).unsqueeze(0).mul(2).sub(1)
        if upsample:
            small = source.resize(((image_size + width_offset) // 4, (image_size + height_offset) // 4))
            low_res_tensor = th.from_numpy(np.array(small)).float().div(255).permute(2, 0, 1).to(device).unsqueeze(0).mul(2).sub(1)
        if ilvr_spec is not None:  # at the run's frame, as the style image
            pil = source.resize((image_size + width_offset, image_size + height_offset), Image.LANCZOS)
            ilvr_tensor = th.from_numpy(np.array(pil)).float().div(255).permute(2, 0, 1).to(device).unsqueeze(0).mul(2).sub(1)
        if mask_image is not None:
            pil = Image.open(script_util.fetch(mask_image)).convert("L").resize((image_size, image_size))
            mask_tensor = th.from_numpy(np.array(pil)).float().div(255).to(device)[None, None]

    style_tensor = None
    if style_spec is not None:  # at the run's frame; every rank of a sharded run computes the style Gram matrices itself (no collective)
        import numpy as np
        from PIL import Image
        pil = Image.open(script_util.fetch(style_spec[0])).convert("RGB").resize((image_size + width_offset, image_size + height_offset),
                                                                                 Image.LANCZOS)
        style_tensor = th.from_numpy(np.array(pil)).float().div(255).permute(2, 0, 1).to(device).unsqueeze(0).mul(2).sub(1)

    # Multi-GPU (cgd_amd.launch: one process per GPU, torch.distributed initialised): the batch is sharded by samples, one (or
    # a contiguous block) per rank; every rank draws the GLOBAL random tensors from the same seed and keeps its rows, so the
    # frames are those of the single-process batched run.  No per-step collective.
    rank, nranks = shard.world()
    mine = shard.rank_samples(batch_size) if nranks > 1 else list(range(batch_size))
    local_batch = len(mine)
    model_kwargs = {}
    if class_cond:
        model_kwargs["y"] = th.zeros([local_batch], device=device, dtype=th.long)

    if upsample:
        # one image for the whole batch (the handle broadcasts it); the sampler hands it to the model once per loop
        model_kwargs["low_res"] = low_res_tensor
        gd_model, diffusion = script_util.load_upsampler(
            checkpoint_path=diffusion_path, large_size=image_size, diffusion_steps=diffusion_steps, timestep_respacing=timestep_respacing,
            device=device, noise_schedule=noise_schedule, dropout=dropout)
    elif model_spec is not None:
        gd_model, diffusion = script_util.load_community_model(
            model_spec, image_size=image_size, class_cond=class_cond, diffusion_steps=diffusion_steps, timestep_respacing=timestep_respacing,
            device=device, noise_schedule=noise_schedule, checkpoints_dir=str(checkpoints_dir))
    else:
        gd_model, diffusion = script_util.load_guided_diffusion(
            checkpoint_path=diffusion_path, image_size=image_size, class_cond=class_cond, diffusion_steps=diffusion_steps,
            timestep_respacing=timestep_respacing, use_fp16=True, device=device, noise_schedule=noise_schedule, dropout=dropout)
    if windows_spec is not None:  # ClipGuidance and the loop see the wrapper; the loader's cache keeps the bare handle
        gd_model = nets.WindowedUNet(gd_model, stride=windows_spec[0], wrap=windows_spec[1], feather=windows_spec[2])
    # (a collective like the loads above: before the early return of a rank without samples)
    secondary = clip_util.load_secondary(gd_model.ctx, secondary_path, device) if secondary_path is not None else None
    aesthetic_kw = {}
    if any(spec is not None for spec in aesthetic_specs):  # (collectives too: one small broadcast per head)
        heads = [None if spec is None else clip_util.load_aesthetic(gd_model.ctx, spec[0], device, cm.tower.out_dim, name)
                 for spec, cm, name in zip(aesthetic_specs, clip_models, clip_names)]
        aesthetic_kw = dict(aesthetic_heads=heads, aesthetic_scale=[0.0 if spec is None else spec[1] for spec in aesthetic_specs])
    classifier = None
    if classifier_spec is not None:  # (a collective too)
        classifier = clip_util.load_classifier(gd_model.ctx, classifier_spec[0], device, image_size)
        if classifier.image_size != image_size:
            raise ValueError(f"{classifier_spec[0]} is the {classifier.image_size}x{classifier.image_size} classifier, the run is {image_size}x{image_size}")
        if not (0 <= classifier_spec[1] < classifier.out_channels):
            raise ValueError(f"classifier=...:{classifier_spec[1]}: CLASS must be in [0, {classifier.out_channels})")
        if class_cond:  # the diffusion model is steered toward the same class for the whole run
            model_kwargs["y"] = th.full([local_batch], classifier_spec[1], device=device, dtype=th.long)
            if randomize_class:
                randomize_class = False
                tqdm.write(f"classifier guidance: y is held at class {classifier_spec[1]} (randomize_class switched off)")

    if local_batch == 0:
        return  # more ranks than samples: this rank only took part in the weight broadcasts above (they are collectives)

    if reduce_clip and skip_timesteps == 0:
        skip_timesteps = int(diffusion.num_timesteps * 0.2)
        if progress:
            tqdm.write(f"--reduce-clip: the first {skip_timesteps} timesteps are skipped")

    invert_kw = {}
    if invert:
        # once, at batch 1, unguided, with class 0 where the model is class-conditional; every sample of the batch starts from that latent.
        # A run reproduces the image only with the class held fixed (--uncond, or randomize_class=False)
        _, inv_noise = diffusion.ddim_invert(gd_model, init_tensor, clip_denoised=False, progress=progress, skip_timesteps=skip_timesteps,
                                             model_kwargs={"y": th.zeros([1], device=device, dtype=th.long)} if class_cond else {})
        invert_kw["noise"] = inv_noise.expand(local_batch, -1, -1, -1).contiguous()

    # every rank of a sharded run builds the same plan; the frame is the sample's, offsets included
    region_plan = regions.plan_from_specs(region_specs, image_size + height_offset, image_size + width_offset, device)
    cond_fn = ClipGuidance(
        gd_model.ctx, gd_model, [cm.tower for cm in clip_models], diffusion, target_embeds, weight_t, num_cutouts, cutout_power=cutout_power,
        clip_guidance_scale=clip_guidance_scale, tv_scale=tv_scale, range_scale=range_scale, sat_scale=sat_scale, use_magnitude=use_magnitude,
        reduce_clip=reduce_clip, progressive_cutout=progressive_cutout, cached_cutouts=cached_cutouts, make_cutouts=make_cutouts,
        # "initialized lazily as it can use a bit of VRAM" (reference cgd.py:146-148): only with an init image and a non-zero scale
        # ... or with a style image, whose term runs on the same trunk
        lpips=script_util.load_lpips(gd_model.ctx, checkpoints_dir, device)
        if ((init_tensor is not None and init_scale != 0) or style_tensor is not None or lpips_for_later) else None,
        init_tensor=init_tensor, init_scale=init_scale,
        **({} if style_tensor is None else {"style_tensor": style_tensor, "style_scale": style_spec[1]}),
        secondary=secondary,
        **({"direction_source": init_tensor, **direction_kw} if direction_kw else {}),
        **({} if region_plan is None else {"regions": region_plan}),
        **aesthetic_kw,
        **({} if classifier is None else {"classifier": classifier, "classifier_scale": classifier_spec[2], "classifier_class": classifier_spec[1]}))
    if nranks > 1:
        cond_fn.shard = diffusion.shard = (mine, batch_size)

    # "plmsN" (PLMS of order 2, spaced like "ddimN") extends what the reference accepts, like the "A+B" CLIP names
    if timestep_respacing.startswith("plms"):
        loop = functools.partial(diffusion.plms_sample_loop_progressive, order=2)
    # "dpmN" / "dpmsdeN" (likewise): DPM-Solver++(2M), deterministic / SDE, on at most N levels uniform in logSNR
    elif timestep_respacing.startswith("dpmsde"):
        loop = functools.partial(diffusion.dpmpp_sample_loop_progressive, order=2, eta=1.0)
    elif timestep_respacing.startswith("dpm"):
        loop = functools.partial(diffusion.dpmpp_sample_loop_progressive, order=2, eta=0.0)
    else:
        loop = diffusion.ddim_sample_loop_progressive if timestep_respacing.startswith("ddim") else diffusion.p_sample_loop_progressive
    if ilvr_spec is not None:
        loop = functools.partial(loop, ilvr=(ilvr_tensor, ilvr_spec[0], script_util.ilvr_stop(ilvr_spec[1], diffusion.num_timesteps)))
    if threshold is not None:  # only with 'dpmN' / 'dpmsdeN' (split_threshold)
        loop = functools.partial(loop, threshold=threshold[0] if threshold[1] is None else threshold)
    return GuidedRun(
        model=gd_model, diffusion=diffusion, cond_fn=cond_fn, loop=loop, model_kwargs=model_kwargs,
        shape=(local_batch, 3, image_size + height_offset, image_size + width_offset), init_tensor=init_tensor, skip_timesteps=skip_timesteps,
        randomize_class=randomize_class, loop_kw={**({} if mask_tensor is None else {"mask": mask_tensor}), **invert_kw}, progress=progress,
        save_frequency=save_frequency, wandb_run=wandb_run, mine=mine, prefix_path=prefix_path, prompts=prompts, clip_model_name=clip_model_name,
        # what a caller that changes the text prompts between runs needs (cgd_amd.animate): the towers' names, the device, every text
        # embedding made so far by (text, tower name), and the image prompts' embeddings per tower with their weights
        clip_names=clip_names, device=device, text_cache=text_cache,
        image_embeds=[e[text_embeds:] for e in embeds_per_tower], image_weights=weights[text_weights:])


# The reference CLI, flag for flag (cgd.py:290-357): "long alias kind default | help".  kind: str / int / float / path, or "flag"
# for store_true switches.  Only names, aliases, types and defaults are contract (tests/golden/reference_host.json).
_CLI_SPEC = f"""
--prompts -txts str "" | text prompts with optional weights, pipe-separated: 'a cat:0.5|a dog:-0.5'; 'TEXT@@REGION[^POWER][:weight]' is a region prompt (direction prompts and --image_prompts entries take '@@REGION' too): REGION is a mask file (white inside, resized to the frame) or a box 'x0,y0,x1,y1' in fractions of the frame, and the prompt acts on every cutout in proportion to the share of REGION the cutout sees, raised to POWER (default 1), e.g. 'a castle on a hill@@0,0,0.5,1|a pine forest@@0.5,0,1,1'; not with use_augs; 'SOURCE CAPTION=>TARGET CAPTION[:weight]' is a direction prompt (needs --init_image): the change of the image's CLIP embedding relative to the init image is steered along the change from the source to the target caption (e.g. 'a photo of a cat=>a photo of a dog:1.5'); weights of all prompts are normalised together
--image_prompts -imgs str "" | image prompts (paths or URLs) with optional weights, pipe-separated; 'FILE@@REGION[^POWER][:weight]' confines an image prompt to a region as on --prompts (every embedding of the image gets it); one entry may be 'style=FILE[:SCALE]' (no '@@' there): FILE is then no CLIP prompt but the style image of the VGG16 Gram-matrix style loss (texture and palette statistics of relu1_2 .. relu4_3, Gatys / Johnson), resized to the frame, SCALE the weight of that loss (default 1, positive; it does not enter the prompt weights); frame sides must be multiples of 16; works with or without prompts and with --init_image / --init_scale
--image_size -size int 128 | resolution of the diffusion checkpoint: 64, 128, 256 or 512
--init_image -init str "" | start from this image (needs --skip_timesteps); IMAGE::MASK regenerates the white part of MASK and keeps the black part of IMAGE; invert=IMAGE (or invert=IMAGE::MASK, with -respace ddimN / plmsN / dpmN) starts from the DDIM-inverted latent of IMAGE; upsample=IMAGE (or upsample=IMAGE::MASK, with --image_size 256 or 512, not with --uncond or invert=) runs the 64->256 / 128->512 super-resolution checkpoint conditioned on IMAGE at a quarter of the frame, IMAGE at the full frame staying the init image; ilvrN=IMAGE or ilvrN@U=IMAGE (N a power of two in [2, 64] that divides both frame sides, U in (0, 1], default 1; not with ::MASK, invert= or upsample=) conditions sampling on the low frequencies of IMAGE (ILVR): after every step of the first fraction U of the run the band that survives a resize down by N and back up is replaced by that of IMAGE noised to the step's level, IMAGE staying the init image; in every form IMAGE is also the source image of 'SOURCE=>TARGET' direction prompts
--init_scale -is int 0 | weight of the LPIPS-VGG16 term that keeps the sample close to the init image
--skip_timesteps -skip int 0 | how many of the (respaced) timesteps to skip at the noisy end
--prefix -dir path outputs | directory for the PNG frames
--checkpoints_dir -ckpts path {script_util.CACHE_PATH} | where the diffusion / CLIP / LPIPS checkpoints live
--batch_size -bs int 1 | samples per run
--clip_guidance_scale -cgs float 1000 | weight of the CLIP spherical-distance loss
--tv_scale -tvs float 150.0 | weight of the total-variation (smoothness) loss
--range_scale -rs float 50.0 | weight of the out-of-range penalty on the predicted image
--sat_scale -sats float 0.0 | weight of the saturation penalty (useful with ddim)
--seed -seed int 0 | RNG seed
--save_frequency -freq int 1 | write a frame every N steps
--diffusion_steps -steps int 1000 | length of the training schedule
--timestep_respacing -respace str 1000 | number of sampling steps ('250'), 'ddimN', 'plmsN' for PLMS (e.g. -respace plms50), or 'dpmN' / 'dpmsdeN' for DPM-Solver++(2M) / its SDE form on at most N logSNR-uniform levels (e.g. -respace dpm20); 'dpmN+thr=P' or 'dpmsdeN+thr=P:CAP' adds dynamic thresholding of the guided prediction: per sample it is clamped to its own P-quantile of absolute values s (at least 1, at most CAP) and divided by s (e.g. -respace dpm20+thr=0.995; CAP 1 is the static clip to [-1, 1]); a last suffix '+windows=STRIDE[:wrapx|:wrapy|:wrap][:feather]' (e.g. -respace 250+windows=128:wrapx with --width_offset 256) samples a frame larger than the checkpoint in windows (MultiDiffusion): the model runs on overlapping --image_size windows STRIDE pixels apart (a positive multiple of 8, at most --image_size; frame sides multiples of 8) and their predictions are averaged, with sin^2 weights under :feather; :wrapx / :wrapy / :wrap let windows run over the right / bottom / both edges, so the result tiles seamlessly along that axis (STRIDE must divide its length); not with upsample=, invert= or +classifier=; behind everything else, '+model=FILE[:heads=N|:head_channels=N][:new_order]' (e.g. -respace ddim100+model=pixel_art_diffusion_hard_256.pt with --uncond) samples with a community checkpoint of the classic UNet architecture, FILE as given or under --checkpoints_dir: the architecture is read from the file's tensor shapes, the head count from the table of known files or from heads= / head_channels=; not with upsample=
--num_cutouts -cutn int 16 | random cutouts shown to CLIP per step
--cutout_power -cutpow float 1.0 | exponent of the cutout size distribution
--clip_model -clip str ViT-B/32 | one of {clip_util.CLIP_MODEL_NAMES}, a checkpoint file, ARCH=FILE for an open_clip ViT checkpoint (ARCH: ViT-B-32, ViT-B-16, ViT-L-14, ViT-H-14, optional -quickgelu suffix), 'A+B' to sum two towers, 'A+secondary=FILE' to guide through the secondary model FILE, 'A+classifier=FILE:CLASS[:SCALE]' for classifier guidance toward ImageNet class CLASS with the noisy classifier FILE (weight SCALE, default 1; with a class-conditional model y is held at CLASS; needs zero height / width offsets), 'A+aesthetic=FILE:SCALE' to add the LAION aesthetic predictor FILE (the linear sa_0_4_vit_*_linear.pth heads or the five-layer improved-aesthetic-predictor ones, whose embedding width must be tower A's) on the embeddings of the tower entry before it: the loss gains -SCALE times the mean predicted score of the cutouts, a negative SCALE steers away, each tower takes at most one (the list is split on '+': a checkpoint whose own name contains '+', as sac+logos+ava1-l14-linearMSE.pth does, has to be renamed or symlinked), or 'A+cuts=OV:IN' (or 'cuts=OV:IN/OV2:IN2': the second pair once 40 percent of the run is done) for OV whole-frame and IN random cutouts per step through the antialiased cubic resize (--num_cutouts then only affects image prompts)
--uncond -uncond flag | use the unconditional 256 / 512 checkpoints
--noise_schedule -sched str linear | 'linear' or 'cosine'
--dropout -drop float 0.0 | dropout of the diffusion model (inference: keep 0)
--device -dev str "" | 'cuda[:N]' (the MI355X); empty = pick automatically
--wandb_project -proj none | log to this Weights & Biases project
--wandb_entity -ent none | Weights & Biases team / entity
--height_offset -ht int 0 | extra image height in pixels
--width_offset -wd int 0 | extra image width in pixels
--use_augs -augs flag | accepted and ignored, as in the reference
--use_magnitude -mag flag | accepted and ignored, as in the reference
--quiet -q flag | no progress output
--save-as-gif -gif flag | assemble the frames into a GIF with ffmpeg and delete them
--save-as-video -mp4 flag | assemble the frames into an MP4 with ffmpeg and delete them
--reduce-clip -reduce flag | skip the first fifth of the steps, then guide every 4th step until 70 percent are done
--progressive-cutout -cutn_skip flag | cutn/4, then cutn/2, then cutn cutouts as sampling proceeds
--cached-cutouts -cached_cutn flag | draw the cutout boxes once and reuse them
"""
_KINDS = {"str": str, "int": int, "float": float, "path": Path}


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    for line in _CLI_SPEC.strip().splitlines():
        spec, text = (part.strip() for part in line.split("|", 1))
        text = text.replace("%", "%%")  # argparse %-formats help strings
        long_flag, alias, kind, *default = spec.split(None, 3)  # the default may contain spaces (a cache path)
        if kind == "flag":
            parser.add_argument(long_flag, alias, action="store_true", help=text)
        elif kind == "none":
            parser.add_argument(long_flag, alias, default=None, help=text)
        else:
            value = default[0].strip('"')
            if kind in ("int", "float"):  # the literal as written: the reference gives --clip_guidance_scale type=float, default=1000
                value = int(value) if value.lstrip("-").isdigit() else float(value)
            parser.add_argument(long_flag, alias, type=_KINDS[kind], default=value, help=text)
    return parser


# CLI destination -> generator keyword where the two differ; everything else passes through under its own name
_RENAMED = {"prefix": "prefix_path", "clip_model": "clip_model_name"}
_NOT_FORWARDED = ("uncond", "quiet", "save_as_gif", "save_as_video", "use_augs", "use_magnitude")


def kwargs_from_args(args):
    """CLI namespace -> generator kwargs.  Reference quirks kept: `--use_augs/--use_magnitude` are parsed but passed as False
    (cgd.py:402-403), `randomize_class` follows class conditioning (:381), prompt strings split on the pipe character."""
    kw = {_RENAMED.get(name, name): value for name, value in vars(args).items() if name not in _NOT_FORWARDED}
    for key in ("prompts", "image_prompts"):
        kw[key] = kw[key].split("|") if kw[key] else []
    kw.update(class_cond=not args.uncond, randomize_class=not args.uncond, progress=not args.quiet, use_augs=False, use_magnitude=False)
    return kw


def main():
    args = build_parser().parse_args()
    Path(args.prefix).mkdir(exist_ok=True)
    kwargs = kwargs_from_args(args)
    list(enumerate(clip_guided_diffusion(**kwargs)))
    if args.save_as_gif or args.save_as_video:
        import shutil
        import subprocess
        if shutil.which("ffmpeg") is None:
            raise RuntimeError("--save-as-gif/--save-as-video need ffmpeg on PATH")
        _, nranks = shard.world()
        for batch_idx in (shard.rank_samples(args.batch_size) if nranks > 1 else range(args.batch_size)):
            # file names and encoder settings of the reference (script_util.py:104-214): <frames_dir>_<batch_idx:02>.gif|.mp4
            frames_dir = script_util.clean_and_combine_prompts(args.prefix, kwargs["prompts"], batch_idx)
            pattern = f"{frames_dir}/%04d.png"
            if args.save_as_gif:
                palette = f"{frames_dir}/palette.png"
                subprocess.check_call(["ffmpeg", "-y", "-framerate", "10", "-i", pattern, "-vf", "palettegen=max_colors=256:stats_mode=full",
                                       palette])
                subprocess.check_call(["ffmpeg", "-y", "-framerate", "10", "-i", pattern, "-i", palette, "-lavfi",
                                       "paletteuse=dither=floyd_steinberg:bayer_scale=5:diff_mode=rectangle", "-loop", "0",
                                       f"{frames_dir}_{batch_idx:02}.gif"])
                Path(palette).unlink(missing_ok=True)
            if args.save_as_video:
                subprocess.check_call(["ffmpeg", "-y", "-framerate", "10", "-i", pattern, "-c:v", "libx264", "-preset", "slow", "-crf", "18",
                                       "-pix_fmt", "yuv420p", "-movflags", "+faststart", f"{frames_dir}_{batch_idx:02}.mp4"])
            for f in sorted(glob.glob(f"{frames_dir}/*.png")):
                Path(f).unlink()
            if Path(frames_dir).is_dir() and not list(Path(frames_dir).iterdir()):
                Path(frames_dir).rmdir()


if __name__ == "__main__":
    main()
