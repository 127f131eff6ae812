"""WGAN-GP losses with the reference's call signatures (its wgan_gp_loss.py).

``wgan_gp_D_loss(D, G, real, latents, ...) -> (D_cost, D_real_loss, D_fake_loss)`` and
``wgan_gp_G_loss(G, D, latents) -> G_cost`` return device tensors; ``D_cost.backward()`` /
``G_cost.backward()`` (called by ``Trainer.train``, trainer.py:98,111) run the explicit HIP
backward schedules of ``engine`` and leave the gradients in ``param.grad`` (views of each
network's flat gradient buffer), exactly where ``optimizer.step()`` expects them."""
import torch

from . import engine, graphs, ops, plans

# wgan_gp_loss.py:4-5 keeps module-global scratch; the only state kept here is the injectable RNG.
mixing_factors = None
_seed = None                # [seed, draws so far, torch seed it came from] of the mixing-factor stream; None: seeded from torch's RNG at first use
_use_graphs = 'auto'        # 'auto': launch plans; True: hipGraphs everywhere; False: eager
_use_plans = True           # set through ``enable_plans``; tests/test_e2e_gpu.py and tests/test_collective_gpu.py flip it without dropping the recorded plans
_zero_mix = {}              # (n, device) -> [n, 1] zeros: the mixing factors of R1 (read only)


def enable_graphs(flag=True):
    """How the D-step / G-step schedules are issued whenever alpha == 1:
    ``'auto'`` (default): every stage is replayed from a recorded LAUNCH PLAN (plans.py: the same kernels on the same streams with the
    same events as the eager path, minus the Python between them; ``enable_plans(False)`` turns that off) -- the 4x4 stage included
    (minibatch 16, ms per step hipGraph | plan: 1.121 | 0.924; with a one-rank RCCL communicator 4.09 | 1.09 -- a graph replay serialises
    the streams and cannot carry the bucket collectives);
    ``True``: hipGraph replay everywhere (measured slower from 8x8 on: the replay serialises the weight-gradient stream);
    ``False``: eager launches (per-launch instrumentation, debugging)."""
    global _use_graphs
    _use_graphs = 'auto' if flag == 'auto' else bool(flag)
    if not flag:
        graphs.clear()
        plans.clear()


def enable_plans(flag=True):
    """Launch-plan replay of every stage (see ``enable_graphs``).  Under data parallelism the bucket collectives of the
    sweep are part of the plan (the library's RCCL communicator); Trainer turns plans off only when the reduction goes through
    torch.distributed (CPU hosts)."""
    global _use_plans
    _use_plans = bool(flag)
    if not flag:
        plans.clear()


def _replay_mode(net):
    """'graph' | 'plan' | None (eager) for a step of ``net`` at its current growth stage (alpha == 1 is checked by the callers)."""
    if _use_graphs is False:
        return None
    if _use_graphs is True:
        return 'graph'
    return 'plan' if _use_plans else None


def set_mixing_factors(m):
    """Inject the U[0,1) draw of wgan_gp_loss.py:15-17 for the NEXT wgan_gp_D_loss call (parity tests)."""
    global mixing_factors
    mixing_factors = m


def manual_seed(seed, device='cuda'):
    """Seed the stream the mixing factors are drawn from (counter-based: ``pg_uniform_f32(seed, draw number, element)``).
    Without this call the stream follows ``torch.manual_seed``: it is (re)seeded from ``torch.initial_seed()`` at first use and
    again whenever that value has changed since (two same-seed runs in one process draw the same factors)."""
    global _seed
    _seed = [int(seed), 0, None]


def _draw_mixing_factors(n, device):
    """U[0,1) [n, 1] on the device (wgan_gp_loss.py:15-17) by the library's own generator: no ATen RNG launch inside the step."""
    global _seed
    ts = int(torch.initial_seed())
    if _seed is None or (_seed[2] is not None and _seed[2] != ts):   # [seed, draws so far, torch seed it was derived from (None: manual_seed)]
        _seed = [ts, 0, ts]
    mix = torch.empty((n, 1), device=device, dtype=torch.float32)
    if mix.is_cuda:
        ops.uniform_(mix, _seed[0], _seed[1])
    else:                                                                # (host emulation in the CPU test-suite only)
        mix.copy_(torch.rand((n, 1), generator=torch.Generator().manual_seed((_seed[0] * 1000003 + _seed[1]) % (1 << 63))))
    _seed[1] += 1
    return mix


class LossTensor(torch.Tensor):
    """A scalar device tensor whose ``backward()`` launches an explicit HIP backward schedule."""

    @staticmethod
    def wrap(t, backward_fn):
        out = torch.Tensor._make_subclass(LossTensor, t)
        out._pg_backward = backward_fn
        return out

    def backward(self, gradient=None, retain_graph=None, create_graph=False, inputs=None):
        if create_graph:
            raise NotImplementedError('third-order differentiation is not part of the path')
        fn = getattr(self, '_pg_backward', None)
        if fn is None:
            raise RuntimeError('backward() was already consumed (or this tensor is a derived copy)')
        scale = 1.0 if gradient is None else float(gradient)
        fn(scale)
        if not retain_graph:
            self._pg_backward = None

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        # derived tensors (``.mean()``, ``.item()`` ...) are plain tensors
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **(kwargs or {}))


def _replayed_backward(net):
    """``backward()`` of a loss whose step was replayed (hipGraph or launch plan): the gradient launches are already enqueued.  A
    replayed plan leaves the weight-gradient stream un-joined; the join happens HERE, so that ``loss.backward(); optimizer.step()``
    keeps the contract of the eager path (engine.d_loss_backward: gradients complete for whatever the caller does next on this
    stream) -- unless the caller has set ``net._rt.skip_join`` (Trainer: the update follows on the weight-gradient stream itself).
    A ``gradient`` other than 1 rescales the flat gradient buffer afterwards, as the eager path does."""
    def fn(scale):
        if not (net._rt.skip_join and scale == 1.0):
            engine._join_side()
        net._rt.plan_unjoined = False        # joined, or the caller took over (its update is ordered behind the weight-gradient stream)
        if scale != 1.0:
            ops.axpby_mask(net._flat_grad, a=scale, out=net._flat_grad)
    return fn


def _mixing_factors(penalty, n, device):
    """[n, 1] on the device for a step with a penalty.  'r1' (the penalty at the real images): cached zeros -- neither the injected tensor
    nor the stream of draws is touched; 'gp': the injected tensor, consumed, or else a draw (:15-17, device RNG)."""
    global mixing_factors
    if penalty == 'r1':
        key = (n, str(device))
        if key not in _zero_mix:
            _zero_mix[key] = torch.zeros((n, 1), device=device, dtype=torch.float32)
        return _zero_mix[key]
    if mixing_factors is None:
        return _draw_mixing_factors(n, device)
    mix, mixing_factors = mixing_factors.to(device=device, dtype=torch.float32).reshape(n, 1), None
    return mix


def _step_mode(net, D, x):
    """'graph' | 'plan' | None (eager) for a step of ``net`` on the input ``x``: THE condition under which a step may be replayed."""
    if not (float(net.alpha) >= 1.0 and x.is_cuda and hasattr(net, '_flat_param') and D._rt.global_stddev is None):
        return None                                                      # (exact-global stddev: collectives inside the step -> eager)
    mode = _replay_mode(net)
    ex = net._rt.grad_exchange if net._rt.grad_hook is not None else None
    # (bench.py times every collective with a fresh HIP event pair, ``DataParallel.record_events``: those steps are issued eagerly)
    return None if (mode == 'plan' and ex is not None and ex.dp.record_events) else mode


def _d_loss(objective, D, G, real_images_in, fake_latents_in, return_all):
    """reference wgan_gp_loss.py:36-65 with the loss block and penalty of ``objective`` (engine.Objective).  With an Augmenter the step's
    parameter table (2N rows: reals, then fakes) is made HERE, eagerly -- the uniforms launch and the table launch, outside every plan and
    graph -- and handed down beside the mixing factors."""
    D.zero_grad()                                                        # :42
    G.zero_grad()                                                        # :43
    table = None
    if objective.augment is not None:
        table = objective.augment.next_table('d', 2 * real_images_in.size(0), real_images_in.size(2), real_images_in.size(3))
    mix = mode = None                                                    # no penalty: one pass over [real | fake], eager in every mode
    if objective.penalty is not None:
        mix = _mixing_factors(objective.penalty, real_images_in.size(0), real_images_in.device)
        mode = _step_mode(D, D, real_images_in)
    if mode is None:
        d_cost, d_real_loss, d_fake_loss, state = engine.d_loss_forward(D, G, real_images_in, fake_latents_in, mix, objective, table)
        d_cost = LossTensor.wrap(d_cost, lambda scale: engine.d_loss_backward(state, scale))
    else:
        d_cost, d_real_loss, d_fake_loss = (graphs if mode == 'graph' else plans).d_step(
            D, G, engine._check_dev(real_images_in, 'real images'), engine._check_dev(fake_latents_in, 'latents'), mix.contiguous(), objective, table)
        d_cost = LossTensor.wrap(d_cost, _replayed_backward(D))  # gradients are already in param.grad
    return (d_cost, d_real_loss, d_fake_loss) if return_all else d_cost


def _g_loss(objective, G, D, fake_latents_in):
    """reference wgan_gp_loss.py:68-74 with the generator term of ``objective``."""
    G.zero_grad()                                                        # :69
    table = None
    if objective.augment is not None:                                    # (N rows, drawn eagerly from the G stream of the Augmenter: as in _d_loss)
        r = 4 * 2 ** int(G.depth)
        table = objective.augment.next_table('g', fake_latents_in.size(0), r, r)
    mode = _step_mode(G, D, fake_latents_in)
    if mode is None:
        g_cost, state = engine.g_loss_forward(G, D, fake_latents_in, objective, table)
        return LossTensor.wrap(g_cost, lambda scale: engine.g_loss_backward(state, scale))
    g_cost = (graphs if mode == 'graph' else plans).g_step(G, D, engine._check_dev(fake_latents_in, 'latents'), objective, table)
    return LossTensor.wrap(g_cost, _replayed_backward(G))


def wgan_gp_D_loss(D, G, real_images_in, fake_latents_in, iwass_lambda=10.0, iwass_epsilon=0.001, iwass_target=1.0, return_all=True):
    """reference wgan_gp_loss.py:36-65, on the original loss kernels (the 'original' family of engine.Objective)."""
    obj = engine.WGAN_GP                                                 # (the default arguments build nothing)
    if iwass_lambda != obj.weight or iwass_epsilon != obj.drift or iwass_target != obj.target:
        obj = obj._replace(drift=iwass_epsilon, weight=iwass_lambda, target=iwass_target)
    return _d_loss(obj, D, G, real_images_in, fake_latents_in, return_all)


def wgan_gp_G_loss(G, D, fake_latents_in):
    """reference wgan_gp_loss.py:68-74."""
    return _g_loss(engine.WGAN_GP, G, D, fake_latents_in)
