"""Run-time state of one network's step schedules: everything ``engine`` / ``plans`` / ``trainer`` keep ON a network between launches.
``_FlatParamsMixin`` owns one ``NetRuntime`` per network as ``net._rt``: created with the flat parameter buffer, left out of pickles, fresh
after a reload.  The class is closed: a schedule feature that needs a new piece of state declares it here.  Imports nothing from the package."""


class NetRuntime(object):
    __slots__ = ('derived_ver', 'derived_live', 'derived_ev', 'derived_waited', 'derived_bwd_ev', 'derived_bwd_waited', 'bwd_wanted',
                 'defer_active', 'pending_ev', 'pending', 'skip_join', 'plan_unjoined', 'grad_hook', 'grad_exchange',
                 'global_stddev', 'gs_checked', 'early_g_request', 'early_fwd', 'd_fwd_buffers', 'ema_ev')

    def __init__(self):
        # ---- derived weights: written by engine._derived; plans._prologue re-checks the version before a replay
        self.derived_ver = None             # (param version, depth) of the last refresh; None = stale (reset_derived, first request of a layer)
        self.derived_live = frozenset()     # ids of the conv layers that refresh covered; read by engine._assert_live
        self.derived_ev = None              # event behind its forward forms; waited for by _await_derived / order_side_behind_derived
        self.derived_waited = set()         # ... stream handles already ordered behind it
        self.derived_bwd_ev = None          # event behind its backward-only copies; waited for by engine._await_backward_copies
        self.derived_bwd_waited = set()     # ... stream handles already ordered behind it
        self.bwd_wanted = False             # set by the first backward sweep (_want_backward_copies): every refresh includes the backward copies
        # ---- deferred update
        self.defer_active = False           # engine.defer_to_side is running the update: _derived closes it behind the forward forms ...
        self.pending_ev = None              # ... with this event, which defer_to_side takes
        self.pending = None                 # event of a deferred update nobody waited for yet; taken by engine.wait_pending / plans' PENDING entries
        # ---- join protocol of the weight-gradient stream
        self.skip_join = False              # Trainer / plans.d_step: the caller orders its update behind the weight gradients; read by backward()
        self.plan_unjoined = False          # plans.d_step left that stream un-joined; cleared by wgan_gp_loss._replayed_backward
        # ---- gradient exchange under data parallelism: installed by Trainer._open_exchange, hook cleared by Trainer after backward()
        self.grad_hook = None               # GradExchange.ready; called by engine._grads_ready as blocks of a sweep complete
        self.grad_exchange = None           # the GradExchange; finished by parallel.all_reduce_grads, part of a plan's key
        # ---- minibatch-stddev mode (Discriminator)
        self.global_stddev = None           # Trainer: the data-parallel group in the exact-global mode; None = local-shard statistics (engine._mbstd_*)
        self.gs_checked = None              # (batch, groups) engine._mbstd_fwd last verified to be equal on all ranks
        # ---- early generator pass
        self.early_g_request = None         # on D: (G, latents) of the coming G step (engine.request_early_g); taken by the D step
        self.early_fwd = None               # on G: the engine.EarlyG the D step left; taken by the G step (engine.take_early_g, plans.g_step)
        # ---- three-pass D forward
        self.d_fwd_buffers = None           # engine._DForwardBuffers of the current (stage, shape); graphs.d_step keeps them alive
        # ---- smoothed generator (on G)
        self.ema_ev = None                  # event behind the last second-stream launch of ema.GeneratorEMA.update, which writes it (None: inline);
        #                                     waited for by the stream of G's next parameter update (Trainer, before optimizer_g.step(): the launch
        #                                     READS G's parameters) and by GeneratorEMA.network() (its consumers read what the launch wrote)

    def reset_derived(self):
        self.derived_ver = None

    def take(self, field):
        """Take-and-clear of a hand-over field (pending_ev, early_g_request, early_fwd)."""
        v = getattr(self, field)
        setattr(self, field, None)
        return v


# the same state as loose attributes of the network, as earlier versions pickled it (None / False / empty): dropped from their snapshots on load
LEGACY_KEYS = frozenset('_' + f for f in NetRuntime.__slots__)


def of(net):
    """The run-time object of a product network; None for a foreign module (Trainer accepts any ``D`` / ``G``)."""
    return net.__dict__.get('_rt')
