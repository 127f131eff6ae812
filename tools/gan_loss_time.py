#!/usr/bin/env python
"""Device time of the selectable GAN objectives (gan_losses.py): per D step and per full Trainer iteration.

    python tools/gan_loss_time.py [--stage 1024x3 128x16] [--rounds 3] [--prime 12] [--steps 30] [--windows 3]

Cases: WGAN-GP (``wgan_gp_D_loss`` / ``wgan_gp_G_loss``: today's functions, the same code as before the feature), the same two functions
behind wrappers ("foreign": what Trainer's deferred D update and early generator pass, which are keyed to those function objects, are
worth), 'logistic' + 'r1', 'logistic' + 'gp' (both on the three-pass schedule, replayed from launch plans) and 'hinge' without a
penalty (the one-pass schedule, eager).  A stage is ``<resolution>x<minibatch>`` of the default 1024x1024 network pair.  One process per invocation; per stage the
cases run round by round, interleaved, on the same network pair with Adam at lr 0 (every step on the seeded weights):

  D step     ``c = D_loss(D, G, real, z); c[0].backward()`` -- ``--steps`` of them between two HIP events on the main stream (backward joins
             the weight-gradient stream), after ``--prime`` un-timed ones (past the two eager warm-up steps and the recording of a plan);
  iteration  ``Trainer.train()`` on device-resident synthetic batches, the same way.

Per case: the median over rounds x windows and the spread (max - min) of the windows.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [('wgan-gp', None), ('wgan-gp foreign', 'foreign'), ('logistic+r1', ('logistic', 'r1')), ('logistic+gp', ('logistic', 'gp')),
         ('hinge+none', ('hinge', None))]


def _losses(pg, spec):
    if spec is None:
        return pg.wgan_gp_D_loss, pg.wgan_gp_G_loss
    if spec == 'foreign':
        # WGAN-GP behind two wrappers: the same launches, but Trainer no longer recognises the function objects, so it joins the
        # weight-gradient stream and updates inline, and the G step runs its own generator pass -- how it treats every gan_losses() pair
        return (lambda D, G, real, z: pg.wgan_gp_D_loss(D, G, real, z)), (lambda G, D, z: pg.wgan_gp_G_loss(G, D, z))
    return pg.gan_losses(spec[0], penalty=spec[1], penalty_weight=10.0)


def _window(torch, fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def stage(torch, pg, res, mb, args):
    depth = {4 * 2 ** d: d for d in range(9)}[res]
    torch.manual_seed(1337)
    shape = (1, 3, 1024, 1024)
    G, D = pg.Generator(shape).cuda(), pg.Discriminator(shape).cuda()
    G.depth = D.depth = depth
    ds = pg.utils.SyntheticDataset(res, 3, seed=1337, ring=8)
    ds.model_depth = depth
    real = next(ds.loader(mb))
    z = pg.utils.device_latents(mb, G.latent_size, seed=7)()
    times = {name: {'d_step': [], 'iteration': []} for name, _ in CASES}
    for r in range(args.rounds):
        for name, spec in CASES:
            D_loss, G_loss = _losses(pg, spec)
            pg.wgan_gp_loss.manual_seed(1337)

            def d_step():
                D_loss(D, G, real, z)[0].backward()
            for _ in range(args.prime):
                d_step()
            times[name]['d_step'] += [_window(torch, d_step, args.steps) for _ in range(args.windows)]
            opt_g = pg.FusedAdam(G.parameters(), 0.0, betas=(0.0, 0.99))          # lr 0: every step runs on the seeded weights
            opt_d = pg.FusedAdam(D.parameters(), 0.0, betas=(0.0, 0.99))
            tr = pg.Trainer(D, G, D_loss, G_loss, opt_d, opt_g, ds, ds.loader(mb), pg.utils.device_latents(mb, G.latent_size, seed=1344, ring=16))
            for _ in range(args.prime):
                tr.train()
            times[name]['iteration'] += [_window(torch, tr.train, args.steps) for _ in range(args.windows)]
            print('[gan_loss_time] %dx%d round %d %-12s D step %.3f ms  iteration %.3f ms' % (
                res, mb, r, name, statistics.median(times[name]['d_step'][-args.windows:]),
                statistics.median(times[name]['iteration'][-args.windows:])), flush=True)
    out = {'resolution': res, 'minibatch': mb, 'rounds': args.rounds, 'windows': args.windows, 'steps_per_window': args.steps, 'cases': {}}
    for name, _ in CASES:
        out['cases'][name] = {k: {'median_ms': statistics.median(v), 'spread_ms': max(v) - min(v), 'windows_ms': v} for k, v in times[name].items()}
    base = out['cases']['wgan-gp']
    print('[gan_loss_time] %dx%d  %-12s %21s %21s' % (res, mb, 'case', 'D step ms (spread)', 'iteration ms (spread)'))
    for name, _ in CASES:
        c = out['cases'][name]
        print('[gan_loss_time] %dx%d  %-12s %12.3f (%.3f) %14.3f (%.3f)   x%.3f / x%.3f of WGAN-GP' % (
            res, mb, name, c['d_step']['median_ms'], c['d_step']['spread_ms'], c['iteration']['median_ms'], c['iteration']['spread_ms'],
            c['d_step']['median_ms'] / base['d_step']['median_ms'], c['iteration']['median_ms'] / base['iteration']['median_ms']))
    print(json.dumps(out))
    pg.wgan_gp_loss.enable_graphs(False)            # drop the plans (and the activations they pin) before the next stage
    pg.wgan_gp_loss.enable_graphs('auto')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--stage', nargs='+', default=['1024x3', '128x16'])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--prime', type=int, default=12)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--out', default=None, help='write the JSON of every stage to this file too')
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        sys.exit('gan_loss_time.py needs a GPU')
    import pggan_amd as pg
    results = []
    for s in args.stage:
        res, mb = (int(v) for v in s.split('x'))
        results.append(stage(torch, pg, res, mb, args))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
