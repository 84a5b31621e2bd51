"""Cost of DDIM inversion at the headline shape (bench.py config 2's networks: 256x256, cutn 16, CLIP ViT-B/32, batch 1, synthetic weights;
schedule ddim50), in one process:

  launch_us       microseconds per launch of cgd_ddim_reverse_update (plain, and the last step's form with noise_out) next to
                  cgd_sample_update mode 1, from HIP events around --launch-iters back-to-back launches
  invert_ms       milliseconds per inversion step: ddim_invert over the first 25 levels (UNet forward + one launch per step), wall clock
                  around work that ends in a device synchronise
  guided_ddim_ms  milliseconds per guided DDIM step of ddim_sample_loop_progressive started from the inverted latent, same skip

Every figure is the median of --repeats measurements (taken alternately, after one untimed warm-up) with their minimum and maximum beside it.
Prints one JSON line.  Usage: python benchmarks/invert_step.py [--repeats 5]"""
import argparse
import json
import time

import steplib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launch-iters", type=int, default=500)
    args = ap.parse_args()
    import torch as th
    dev = steplib.DEV
    cfg, ctx, (unet, towers, smp, guid, image) = steplib.setup(spec="ddim50")
    H, W = cfg["hw"]
    y = {"y": th.zeros(1, dtype=th.long, device=dev)}
    skip = smp.num_timesteps // 2
    t0 = smp.num_timesteps - 1 - skip

    def invert():
        th.cuda.synchronize()
        t = time.perf_counter()
        latent, noise = smp.ddim_invert(unet, image, model_kwargs=dict(y), device=dev, skip_timesteps=skip)
        th.cuda.synchronize()
        return (time.perf_counter() - t) / t0 * 1e3, noise, bool(th.isfinite(latent).all())

    def guided(noise):
        guid.current_timestep = smp.num_timesteps - 1
        it = smp.ddim_sample_loop_progressive(unet, (1, 3, H, W), noise=noise, clip_denoised=False, cond_fn=guid, model_kwargs=dict(y),
                                              device=dev, skip_timesteps=skip, init_image=image, randomize_class=False,
                                              cond_fn_with_grad=True)
        t, n, out = steplib.drain(it, guid)
        return t / n * 1e3, n, bool(th.isfinite(out["sample"]).all())

    th.manual_seed(1000)
    _, noise, _ = invert()  # warm-up: buffers, first touch of the kernels
    guided(noise)
    inv_ms, gd_ms, finite = [], [], {}
    for _ in range(args.repeats):
        ms, noise, ok = invert()
        inv_ms.append(ms)
        finite["invert"] = ok
        ms, n_guided, ok = guided(noise)
        gd_ms.append(ms)
        finite["guided_ddim"] = ok

    # per-launch cost at the headline shape
    x, x0, mean, g, nz = (th.randn(1, 3, H, W, device=dev) for _ in range(5))
    out6 = th.randn(1, 6, H, W, device=dev)
    logvar = th.randn_like(x) * 0.1 - 5
    sample, x0_out, noise_out = th.empty_like(x), th.empty_like(x), th.empty_like(x)
    scal = th.ones(8, device=dev)
    k = smp.tables.step_coef(t0, t0)
    rk = smp.tables.reverse_coef(t0 - 1)

    def sample_update():
        ctx.check(ctx.lib.cgd_sample_update(ctx.h, x.data_ptr(), x0.data_ptr(), mean.data_ptr(), logvar.data_ptr(), g.data_ptr(),
                                            nz.data_ptr(), scal.data_ptr(), sample.data_ptr(), x0_out.data_ptr(), 1, H, W, k, 1,
                                            ctx.stream()))

    def reverse(with_noise):
        def fn():
            ctx.check(ctx.lib.cgd_ddim_reverse_update(ctx.h, x.data_ptr(), out6.data_ptr(), image.data_ptr() if with_noise else None,
                                                      sample.data_ptr(), x0_out.data_ptr(), noise_out.data_ptr() if with_noise else None,
                                                      1, H, W, 1, rk, ctx.stream()))
        return fn

    fns = {"cgd_sample_update_mode1": sample_update, "cgd_ddim_reverse_update": reverse(False),
           "cgd_ddim_reverse_update_noise_out": reverse(True)}
    launch = steplib.per_launch(fns, args.launch_iters, args.repeats)
    stat = steplib.stats

    print(json.dumps({"what": "DDIM inversion at 256x256, batch 1, synthetic weights, ddim50, bench.py config 2's networks; median / min / max of "
                              f"{args.repeats} alternating repeats",
                      "launch_us": {n: stat(v, 2) for n, v in launch.items()},
                      "invert_ms_per_step": stat(inv_ms, 3), "guided_ddim_ms_per_step": stat(gd_ms, 3),
                      "invert_steps": t0, "guided_steps": n_guided, "finite": finite, "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
