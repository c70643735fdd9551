"""Policies that run INSIDE the closed-loop rollout (``QuadrupedEnv.rollout_policy``): a small MLP evaluated by a resident policy kernel
on the matrix cores, between the published observation rows and the action mailboxes of ``gq_rollout_closed``'s machinery.

The law and the weight blob are defined in ``csrc/gq_policy_mlp.h``; this module packs a network into that blob (no GPU needed) and
restates the network in float64 for tests.

``GruPolicy`` is the recurrent form - one GRU cell and an MLP head, the hidden state on the device (``QuadrupedEnv.policy_hidden``) - defined
in ``csrc/gq_policy_gru.h``.

``HeightScan`` puts the env's base-following height map into either policy's input row (``csrc/gq_policy_scan.h``).

``ObsHistory`` gives the MLP a memory: the frames of the last policy steps as further columns of its input row, the state on the device
(``QuadrupedEnv.policy_history``), defined in ``csrc/gq_policy_hist.h``.

``ObsNoise`` puts counter-based sensor noise on the observation and scan columns either policy is fed (``csrc/gq_policy_noise.h``)."""
from __future__ import annotations

import numpy as np

from .cabi import GQ_ACT

MAX_LAYERS, MAX_WIDTH, N_ACTIONS = 4, 256, 12


def _kp(k):
    return (k + 3) & ~3


def _np(n):
    return (n + 15) & ~15


def elu64(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))


_ACT64 = dict(none=lambda x: x, relu=lambda x: np.maximum(x, 0.0), elu=elu64, tanh=np.tanh)


class HeightScan:
    """A height scan in a policy's input row: the ``rows x cols`` cells of the env's ``HeightMap(rows, cols, ..., follow_base=True)``, in
    the map's own cell order ``i * cols + j``, between the observation columns and the fed-back action::

        x = [ obs_row[:in_obs] (shift / scale) | scan[0 : rows * cols] | last action (12, with feed_last_action) ]
        scan_c = clamp((z_base - offset) - z_hit_c, -clip, +clip) * scale

    in float32, every operation rounded (``csrc/gq_policy_scan.h``).  ``z_hit_c`` is the z of the cell's hit point (a ray that hits nothing
    saturates at ``-clip``), ``z_base`` the base's z in the env's observation row (``base_pos`` or ``qpos`` must be observed; the column need
    not be one the network reads).  ``obs_shift`` / ``obs_scale`` never act on scan columns: ``offset`` and ``scale`` are the scan's own."""

    default_policy_waves = 256   # an MlpPolicy's rollout (profiles/height_scan_throughput.txt): 16 384 envs gain a quarter over 128, 4096 lose 1 %

    def __init__(self, rows, cols, offset=0.0, clip=1.0, scale=1.0):
        self.rows, self.cols = int(rows), int(cols)
        if self.rows < 1 or self.cols < 1 or self.rows != rows or self.cols != cols:
            raise ValueError(f'a height scan needs rows, cols >= 1, got {rows} x {cols}')
        self.offset, self.clip, self.scale = float(offset), float(clip), float(scale)
        if not all(np.isfinite(v) for v in (self.offset, self.clip, self.scale)):
            raise ValueError(f'offset, clip and scale must be finite, got {offset}, {clip}, {scale}')
        if not self.clip > 0.0:
            raise ValueError(f'clip must be positive, got {clip}')

    @property
    def cells(self):
        return self.rows * self.cols

    def _struct(self):
        import ctypes as C

        from .cabi import GqPolicyScan
        return GqPolicyScan(struct_size=C.sizeof(GqPolicyScan), rows=self.rows, cols=self.cols, offset=self.offset, clip=self.clip, scale=self.scale)


class ObsHistory:
    """A history of past policy inputs in an ``MlpPolicy``'s input row: the FRAMES of the last ``frames`` policy steps behind the fed-back
    action, newest first::

        x = [ obs_row[:in_obs] (shift / scale) | scan (if any) | last action (12, if fed) | frame_1 | ... | frame_L ]

    A frame is what the network was fed as its current block at one policy step, raw: the first ``cols`` observation words (default: all
    ``in_obs``) as loaded and, with ``feed_last_action``, the 12 fed-back action words of that step - ``F = cols + 12 feed_last_action``
    words, ``in_dim = in_obs + cells + 12 f + frames * F <= 256``.  When a frame is fed, ``obs_shift`` / ``obs_scale`` act on its
    observation words by their original column and not on its action words, so ``frame_i`` at policy step ``s`` carries exactly the values
    the current block carried at step ``s - i``.  The weights behind the current block are ordinary first-layer rows.

    In ``rollout_policy`` the frames live in ``env.policy_history`` ``[N, frames, F]`` and follow the GRU's episode rule
    (``csrc/gq_policy_hist.h``): all frames of an env become zero at the policy seat's visit that sees its termination (at the first step of
    a call: that it waits for its re-spawn), so the history fed at policy step ``s + 1`` is zero exactly where ``dones[s]`` is set.  The
    fed-back last action itself is NOT reset with the env: zeros at the first policy step of a call, kept across a re-spawn, as without a
    history - and a frame records it as it was fed."""

    default_policy_waves = 256   # the sweep of profiles/obs_history_throughput.txt: no count is best everywhere, 256 loses the least (go2, 16 384 envs: 14 %)

    def __init__(self, frames, cols=None):
        if int(frames) != frames or int(frames) < 1:
            raise ValueError(f'an observation history needs frames >= 1, got frames = {frames}')
        if cols is not None and (int(cols) != cols or int(cols) < 1):
            raise ValueError(f'an observation history needs 1 <= cols <= in_obs, got cols = {cols}')
        self.frames, self.cols = int(frames), None if cols is None else int(cols)

    def frame_words(self, in_obs, feed_last_action):
        """F: the words of one frame for a policy of ``in_obs`` observation columns"""
        return (in_obs if self.cols is None else self.cols) + (N_ACTIONS if feed_last_action else 0)


class ObsNoise:
    """Sensor noise on what an in-loop policy observes (``rollout_policy(..., obs_noise=)``; ``csrc/gq_policy_noise.h`` is the law), in RAW
    observation units, before ``obs_shift`` / ``obs_scale``::

        o~_c = o_c + amp[c] * n      observation column c < in_obs with amp[c] > 0
        s~_c = s_c + scan_amp * n    scan column (the scan word after clamp and scale, from the true z), with scan_amp > 0

    in float32, the product and the sum each rounded.  ``kind='uniform'``: ``n = 2 u - 1`` in ``[-1, 1)``; ``'normal'``: a standard normal, the
    action noise's Box-Muller.  The draw is counter-based - a Philox block per word keyed by the env's seed, the input-row column, the step
    counter of the policy step and the global env id - so a seed gives one rollout and two shards draw different noise.  A column with
    amplitude 0 draws nothing and keeps its bits.  The fed-back action and a history's frames are never noised: a frame holds the noisy word
    its current block was fed.  Only the network's input is noised - the joint-impedance law, the reward and the episode rules read the true
    row.

    amp: a scalar or ``[policy.in_obs]`` non-negative finite values (``from_names`` fills it by observation name); scan_amp: one
    non-negative amplitude for every column of the policy's ``HeightScan`` (refused when non-zero and the policy has none)."""

    KINDS = ('uniform', 'normal')

    def __init__(self, amp, kind='uniform', scan_amp=0.0):
        if kind not in self.KINDS:
            raise ValueError(f"kind must be 'uniform' or 'normal', got {kind!r}")
        self.kind = kind
        self.amp = np.array(amp, dtype=np.float32)
        if self.amp.ndim > 1:
            raise ValueError(f'amp must be a scalar or a vector of one amplitude per observation column, got shape {self.amp.shape}')
        if not np.all(np.isfinite(self.amp)) or np.any(self.amp < 0):
            raise ValueError('amp must be finite and >= 0 (non-negative amplitudes in raw observation units)')
        self.scan_amp = float(np.float32(scan_amp))
        if not np.isfinite(self.scan_amp) or self.scan_amp < 0:
            raise ValueError(f'scan_amp must be finite and >= 0, got {scan_amp}')
        self._device = {}   # (device, in_obs) -> the amplitude table

    @classmethod
    def from_names(cls, env, amps, kind='uniform', scan_amp=0.0):
        """``amps``: ``{observation name: a scalar or one value per column of that observation}`` in the column layout of ``env``'s
        ``state_obs_names``; every other column gets 0.  A name the env does not observe raises."""
        from .cabi import OBS_DIMS, OBS_NAMES
        names = list(env.state_obs_names)
        unknown = [n for n in amps if n not in names]
        if unknown:
            raise ValueError(f'{unknown} not in the env\'s state_obs_names {names}: only an observed column can be noised')
        parts = []
        for n in names:
            w = OBS_DIMS[OBS_NAMES.index(n)]
            parts.append(np.broadcast_to(np.asarray(amps.get(n, 0.0), dtype=np.float32), (w,)))
        noise = cls(np.concatenate(parts), kind=kind, scan_amp=scan_amp)
        noise._whole_row = True
        return noise

    _whole_row = False   # from_names: amp covers the env's whole row, of which a policy may read the leading columns only

    def table(self, policy):
        """the ``[policy.in_obs]`` float32 amplitudes for ``policy``.  A vector must have ``in_obs`` values; ``from_names``' amplitudes cover
        the env's whole row and are cut to the columns the policy reads - a noised column behind them raises."""
        n = int(policy.in_obs)
        if self.amp.ndim == 0:
            return np.full(n, self.amp, dtype=np.float32)
        if self._whole_row and self.amp.shape[0] >= n:
            if self.amp[n:].any():
                raise ValueError(f'an observation with noise lies behind the in_obs = {n} columns the policy reads')
        elif self.amp.shape[0] != n:
            raise ValueError(f'amp has {self.amp.shape[0]} values, the policy reads in_obs = {n} observation columns')
        return np.ascontiguousarray(self.amp[:n])

    def _check(self, policy):
        if self.scan_amp != 0.0 and getattr(policy, 'height_scan', None) is None:
            raise ValueError(f'scan_amp = {self.scan_amp} and the policy has no height scan')
        return self.table(policy)

    def _struct(self, policy, device, clean=None):
        """the C block for ``policy`` with the table on ``device``; clean: the tensor of the true rows, or None"""
        import ctypes as C

        import torch

        from .cabi import GQ_OBS_NOISE, GqPolicyNoise
        tab = self._check(policy)
        key = (str(device), tab.shape[0])
        if key not in self._device:
            self._device[key] = torch.from_numpy(tab.copy()).to(device)
        t = self._device[key]
        return GqPolicyNoise(struct_size=C.sizeof(GqPolicyNoise), kind=GQ_OBS_NOISE[self.kind], n_amp=tab.shape[0], scan_amp=self.scan_amp,
                             amp=t.data_ptr(), policy_obs_clean=None if clean is None else clean.data_ptr())


def _scan_split(in_dim, feed_last_action, height_scan, what, history=None):
    """in_obs of an input row of ``in_dim`` columns: what the scan, the fed-back action and the history leave"""
    if history is not None:
        if not isinstance(history, ObsHistory):
            raise ValueError(f'history must be an ObsHistory, got {type(history).__name__}')
        if height_scan is not None and not isinstance(height_scan, HeightScan):
            raise ValueError(f'height_scan must be a HeightScan, got {type(height_scan).__name__}')
        cells, f12, L = 0 if height_scan is None else height_scan.cells, N_ACTIONS if feed_last_action else 0, history.frames
        if in_dim > MAX_WIDTH:
            raise ValueError(f'{what} has in_dim = {in_dim} inputs with the observation history: 1 to {MAX_WIDTH} are supported')
        if history.cols is None:   # in_dim = in_obs + cells + f12 + L (in_obs + f12)
            in_obs, rest = divmod(in_dim - cells - (L + 1) * f12, L + 1)
        else:
            in_obs, rest = in_dim - cells - f12 - L * (history.cols + f12), 0
        if rest or in_obs < 1:
            raise ValueError(f'{what} has in_dim = {in_dim} inputs: in_obs + {cells} scan cells + {f12} + {L} frames of (cols + {f12}) words leaves no in_obs >= 1')
        if history.cols is not None and history.cols > in_obs:
            raise ValueError(f'the observation history has cols = {history.cols}, the policy in_obs = {in_obs}: 1 <= cols <= in_obs')
        return in_obs
    if height_scan is not None and not isinstance(height_scan, HeightScan):
        raise ValueError(f'height_scan must be a HeightScan, got {type(height_scan).__name__}')
    cells = 0 if height_scan is None else height_scan.cells
    in_obs = in_dim - cells - (N_ACTIONS if feed_last_action else 0)
    if in_obs < 0 and not cells:
        raise ValueError(f'feed_last_action needs at least {N_ACTIONS} inputs, {what} has {in_dim}')
    if in_obs < 0:
        raise ValueError(f'a height scan of {cells} cells{" and feed_last_action" if feed_last_action else ""} need at least {in_dim - in_obs} inputs, {what} has {in_dim}')
    return in_obs


def _device_tables(policy, device, rows_given):
    """(blob, shift, scale, in_obs) of ``policy`` on ``device``.  rows_given (``policy_eval``: the rows are the full input rows and no scan block
    travels with the call): a policy with a scan counts its scan columns as given columns - ``in_obs`` grows by them and the tables are
    continued with shift 0 and scale 1, which leave every float32 as it is."""
    import torch
    key = str(device)
    up = lambda v: None if v is None else torch.from_numpy(v).to(device)
    if key not in policy._device:
        policy._device[key] = (up(policy.pack()), up(policy.obs_shift), up(policy.obs_scale))
    blob, shift, scale = policy._device[key]
    cells = policy.height_scan.cells if rows_given and policy.height_scan is not None else 0
    hist = getattr(policy, 'history', None) if rows_given else None
    if not cells and hist is None:
        return blob, shift, scale, policy.in_obs
    # a history's frames are given columns too: their observation words keep the shift / scale of their original column, the fed-back action
    # between the current block and the frames passes unchanged; with feed_last_action the row's last 12 words are the oldest frame's action
    f12 = N_ACTIONS if policy.feed_last_action else 0
    given = policy.in_obs + cells if hist is None else policy.in_dim - f12
    if key + ':rows' not in policy._device:
        def pad(v, fill):
            if v is None:
                return None
            same = lambda n: np.full(n, fill, dtype=np.float32)
            parts = [v, same(cells)]
            if hist is not None:
                parts += [same(f12)] + [w for _ in range(hist.frames) for w in (v[:policy.hist_cols], same(f12))]
            return up(np.concatenate(parts)[:given])
        policy._device[key + ':rows'] = (pad(policy.obs_shift, 0.0), pad(policy.obs_scale, 1.0))
    shift, scale = policy._device[key + ':rows']
    return blob, shift, scale, given


class MlpPolicy:
    """An MLP with up to 4 linear layers (at most 3 hidden layers and the output layer), every width and the input width <= 256, 12 outputs
    (joint-target actions in the hinge order of ``qpos[7:]``), fp32 weights.

    weights: one ``[in, out]`` array per layer (``y = x @ W + b``; ``torch.nn.Linear.weight`` is its transpose); biases: one ``[out]``
    array per layer.  activation: 'relu', 'elu' or 'tanh' between the layers; out_activation: None or 'tanh'.  obs_shift / obs_scale:
    optional per-column ``(o - shift) * scale`` on the observation columns the network reads.  feed_last_action: the env's previous
    policy action (12 values, zeros at the first policy step of a rollout call) follows the observation columns in the input row, so the
    first layer has ``in_obs + 12`` inputs.  height_scan: a ``HeightScan`` - its ``rows * cols`` columns stand between the observation columns
    and the fed-back action, so ``in_obs = in_dim - rows * cols - 12 feed_last_action``; shift / scale keep covering the first ``in_obs``.
    history: an ``ObsHistory`` - ``frames`` frames of ``F = cols + 12 feed_last_action`` words follow the fed-back action, so
    ``in_dim = in_obs + rows * cols + 12 feed_last_action + frames * F``; ``hist_cols`` / ``hist_words`` are ``cols`` and ``F`` resolved."""

    def __init__(self, weights, biases, activation='elu', out_activation=None, obs_shift=None, obs_scale=None, feed_last_action=False, height_scan=None,
                 history=None):
        self.weights = [np.ascontiguousarray(w, dtype=np.float32) for w in weights]
        self.biases = [np.ascontiguousarray(b, dtype=np.float32).reshape(-1) for b in biases]
        if not 1 <= len(self.weights) <= MAX_LAYERS:
            raise ValueError(f'{len(self.weights)} linear layers: 1 to {MAX_LAYERS} are supported (3 hidden layers and the output)')
        if len(self.biases) != len(self.weights):
            raise ValueError('one bias vector per weight matrix')
        k = None
        for l, (w, b) in enumerate(zip(self.weights, self.biases)):
            if w.ndim != 2 or b.shape != (w.shape[1],) or (k is not None and w.shape[0] != k):
                raise ValueError(f'layer {l}: weights {w.shape} (expected [in, out] with in = {k}) and bias {b.shape} do not fit')
            if not (1 <= w.shape[0] <= MAX_WIDTH and 1 <= w.shape[1] <= MAX_WIDTH):
                raise ValueError(f'layer {l}: {w.shape[0]} inputs, {w.shape[1]} outputs: 1 to {MAX_WIDTH} are supported')
            k = w.shape[1]
        if k != N_ACTIONS:
            raise ValueError(f'the network has {k} outputs: {N_ACTIONS} (one per hinge) are needed')
        if activation not in ('relu', 'elu', 'tanh'):
            raise ValueError(f"activation must be 'relu', 'elu' or 'tanh', got {activation!r}")
        if out_activation not in (None, 'none', 'tanh'):
            raise ValueError(f"out_activation must be None or 'tanh', got {out_activation!r}")
        self.activation, self.out_activation = activation, out_activation or 'none'
        self.feed_last_action = bool(feed_last_action)
        self.in_dim = self.weights[0].shape[0]
        self.height_scan = height_scan
        self.history = history
        self.in_obs = _scan_split(self.in_dim, self.feed_last_action, height_scan, 'the first layer', history)
        self.hist_cols = self.hist_words = 0
        if history is not None:
            self.hist_cols = self.in_obs if history.cols is None else history.cols
            self.hist_words = history.frame_words(self.in_obs, self.feed_last_action)
        self.widths = [w.shape[1] for w in self.weights]

        def col(v, name):
            if v is None:
                return None
            return np.array(np.broadcast_to(np.asarray(v, dtype=np.float32), (self.in_obs,)), dtype=np.float32)
        self.obs_shift, self.obs_scale = col(obs_shift, 'obs_shift'), col(obs_scale, 'obs_scale')
        self._device = {}   # device -> (blob, shift, scale) tensors

    @classmethod
    def from_torch(cls, module, **kw):
        """From a ``torch.nn.Sequential`` of ``Linear`` layers with ``ReLU``, ``ELU`` (alpha 1) or ``Tanh`` between them (one kind), optionally a
        ``Tanh`` at the end; anything else raises ``ValueError``.  With ``history=`` (``height_scan=``, ``feed_last_action=``) the first
        layer's ``in_features`` must be the ``in_dim`` of ``ObsHistory``'s formula."""
        import torch.nn as nn
        if not isinstance(module, nn.Sequential):
            raise ValueError(f'from_torch takes a torch.nn.Sequential, got {type(module).__name__}')
        names = {nn.ReLU: 'relu', nn.ELU: 'elu', nn.Tanh: 'tanh'}
        weights, biases, acts = [], [], []
        for m in module:
            if isinstance(m, nn.Linear):
                if len(acts) < len(weights):
                    acts.append('none')
                weights.append(m.weight.detach().cpu().numpy().T)
                biases.append(m.bias.detach().cpu().numpy() if m.bias is not None else np.zeros(m.out_features, dtype=np.float32))
            elif type(m) in names and len(acts) == len(weights) - 1:
                if isinstance(m, nn.ELU) and m.alpha != 1.0:
                    raise ValueError(f'ELU with alpha = {m.alpha}: only alpha = 1 is supported')
                acts.append(names[type(m)])
            else:
                raise ValueError(f'unsupported module in the Sequential: {m!r} (Linear with ReLU, ELU or Tanh)')
        if not weights:
            raise ValueError('the Sequential holds no Linear layer')
        if len(acts) < len(weights):
            acts.append('none')
        hidden, out = set(acts[:-1]), acts[-1]
        if len(hidden) > 1 or 'none' in hidden:
            raise ValueError(f'the hidden layers must share one activation out of ReLU, ELU, Tanh; got {acts[:-1]}')
        if out not in ('none', 'tanh'):
            raise ValueError(f'the output layer may be followed by Tanh or nothing, got {out}')
        return cls(weights, biases, activation=hidden.pop() if hidden else 'relu', out_activation=out, **kw)

    def blob_floats(self):
        return sum(_np(w.shape[1]) * (_kp(w.shape[0]) + 1) for w in self.weights)

    def pack(self):
        """The padded blob (float32 numpy), layer after layer: weights ``[Np / 16][Kp / 4][64]`` - word ``l`` of block ``(cb, kb)`` is
        ``w[4 kb + (l >> 4)][16 cb + (l & 15)]`` - then ``Np`` biases; zeros in the padding."""
        parts = []
        for w, b in zip(self.weights, self.biases):
            k, n = w.shape
            kp, npad = _kp(k), _np(n)
            wp = np.zeros((kp, npad), dtype=np.float32)
            wp[:k, :n] = w
            # [kb, kk, cb, oo] -> [cb, kb, kk, oo]
            parts.append(wp.reshape(kp // 4, 4, npad // 16, 16).transpose(2, 0, 1, 3).reshape(-1))
            bp = np.zeros(npad, dtype=np.float32)
            bp[:n] = b
            parts.append(bp)
        return np.ascontiguousarray(np.concatenate(parts))

    def _obs_blocks(self):
        """(first column, words) of every block of the input row that shift / scale act on: the current one, then each frame's"""
        blocks = [(0, self.in_obs)]
        if self.history is not None:
            col0 = self.in_dim - self.history.frames * self.hist_words
            blocks += [(col0 + i * self.hist_words, self.hist_cols) for i in range(self.history.frames)]
        return blocks

    def reference(self, x):
        """float64 forward pass of the same network over rows ``[n, in_dim]`` (shift / scale applied to the first ``in_obs`` columns and to
        the observation words of a history's frames; scan columns and the fed-back action are taken as given)."""
        h = np.array(x, dtype=np.float64).reshape(-1, self.in_dim)
        for c0, n in self._obs_blocks():
            if self.obs_shift is not None:
                h[:, c0:c0 + n] -= self.obs_shift[:n].astype(np.float64)
            if self.obs_scale is not None:
                h[:, c0:c0 + n] *= self.obs_scale[:n].astype(np.float64)
        for l, (w, b) in enumerate(zip(self.weights, self.biases)):
            h = h @ w.astype(np.float64) + b.astype(np.float64)
            h = _ACT64[self.out_activation if l == len(self.weights) - 1 else self.activation](h)
        return h

    # -- the C struct's network part, with the blob on `device`
    def _struct(self, device, rows_given=False):
        import ctypes as C

        from .cabi import GqPolicyMlp
        blob, shift, scale, in_obs = _device_tables(self, device, rows_given)
        m = GqPolicyMlp(struct_size=C.sizeof(GqPolicyMlp), n_layers=len(self.widths), in_obs=in_obs, feed_last_action=int(self.feed_last_action),
                        activation=GQ_ACT[self.activation], out_activation=GQ_ACT[self.out_activation], decimation=1, blob=blob.data_ptr(),
                        blob_floats=blob.numel(), obs_shift=None if shift is None else shift.data_ptr(), obs_scale=None if scale is None else scale.data_ptr())
        m.width = (C.c_int32 * 4)(*(self.widths + [0] * (4 - len(self.widths))))
        return m

    def _hist_struct(self, state, ctl):
        """the history's C block around the env's store: ``state`` ``[N, 2, frames, F]`` float32, ``ctl`` ``[N]`` int32"""
        import ctypes as C

        from .cabi import GqPolicyHist
        return GqPolicyHist(struct_size=C.sizeof(GqPolicyHist), frames=self.history.frames, cols=self.hist_cols, in_dim=self.in_dim, state=state.data_ptr(),
                            ctl=ctl.data_ptr())


MAX_HIDDEN, MAX_HEAD_LAYERS = 128, 3


def sig64(x):
    return 0.5 * np.tanh(0.5 * x) + 0.5


class GruPolicy:
    """A recurrent policy: one GRU cell (``torch.nn.GRUCell``'s law: gates r, z, n, both bias vectors) on the input row, followed by a head -
    an MLP of 1 to 3 linear layers from the hidden state to the 12 joint-target actions.  Limits: input row ``in_dim <= 256`` columns,
    ``1 <= H <= 128`` hidden units, head widths ``<= 256``; fp32 weights.  The law is ``csrc/gq_policy_gru.h``::

        gi = x @ w_ih + b_ih;  gh = h @ w_hh + b_hh                 (columns [0:H] r, [H:2H] z, [2H:3H] n)
        r = sig(gi_r + gh_r);  z = sig(gi_z + gh_z);  n = tanh(gi_n + r * gh_n);  h' = n + z * (h - n);  a = head(h')

    w_ih ``[in, 3H]``, w_hh ``[H, 3H]`` (``GRUCell.weight_ih`` / ``weight_hh`` are their transposes), b_ih, b_hh ``[3H]``; head_weights /
    head_biases: one ``[in, out]`` / ``[out]`` array per head layer (the first has ``H`` inputs, the last 12 outputs); activation /
    out_activation, obs_shift / obs_scale, feed_last_action, height_scan: as for ``MlpPolicy`` (they act on the head's layers and on the cell's
    input row).

    In ``rollout_policy`` the hidden state lives in ``env.policy_hidden`` ``[N, H]`` and follows THE EPISODE RULE: an env's row is zeroed at the
    policy seat's visit that sees its termination (or, at the first step of a call, that it waits for its re-spawn), before any cell
    evaluation - the state fed at policy step ``s + 1`` is zero exactly where ``dones[s]`` is set.  The fed-back last action is not reset
    with the env (zeros at the first policy step of a call, kept across a re-spawn)."""

    default_policy_waves = 128   # the sweep of profiles/gru_policy_throughput.txt: no count is best everywhere, 128 loses the least

    def __init__(self, w_ih, w_hh, b_ih, b_hh, head_weights, head_biases, activation='elu', out_activation=None, obs_shift=None, obs_scale=None,
                 feed_last_action=False, height_scan=None, history=None):
        if history is not None:
            raise ValueError('a GruPolicy takes no history (ObsHistory): its memory is the hidden state; give the history to an MlpPolicy')
        f = lambda v: np.ascontiguousarray(v, dtype=np.float32)
        self.w_ih, self.w_hh, self.b_ih, self.b_hh = f(w_ih), f(w_hh), f(b_ih).reshape(-1), f(b_hh).reshape(-1)
        if self.w_hh.ndim != 2 or self.w_hh.shape[1] != 3 * self.w_hh.shape[0]:
            raise ValueError(f'w_hh must be [H, 3H], got {self.w_hh.shape}')
        H = self.hidden = int(self.w_hh.shape[0])
        if not 1 <= H <= MAX_HIDDEN:
            raise ValueError(f'{H} hidden units: 1 to {MAX_HIDDEN} are supported')
        if self.w_ih.ndim != 2 or self.w_ih.shape[1] != 3 * H or self.b_ih.shape != (3 * H,) or self.b_hh.shape != (3 * H,):
            raise ValueError(f'w_ih must be [in, {3 * H}] and b_ih, b_hh [{3 * H}], got {self.w_ih.shape}, {self.b_ih.shape}, {self.b_hh.shape}')
        self.in_dim = int(self.w_ih.shape[0])
        if not 1 <= self.in_dim <= MAX_WIDTH:
            raise ValueError(f'the cell has {self.in_dim} inputs: 1 to {MAX_WIDTH} are supported')
        self.head_weights = [f(w) for w in head_weights]
        self.head_biases = [f(b).reshape(-1) for b in head_biases]
        if not 1 <= len(self.head_weights) <= MAX_HEAD_LAYERS:
            raise ValueError(f'the head has {len(self.head_weights)} linear layers: 1 to {MAX_HEAD_LAYERS} are supported')
        if len(self.head_biases) != len(self.head_weights):
            raise ValueError('one bias vector per weight matrix of the head')
        k = H
        for l, (w, b) in enumerate(zip(self.head_weights, self.head_biases)):
            if w.ndim != 2 or b.shape != (w.shape[1],) or w.shape[0] != k:
                raise ValueError(f'head layer {l}: weights {w.shape} (expected [in, out] with in = {k}) and bias {b.shape} do not fit')
            if not 1 <= w.shape[1] <= MAX_WIDTH:
                raise ValueError(f'head layer {l}: {w.shape[1]} outputs: 1 to {MAX_WIDTH} are supported')
            k = w.shape[1]
        if k != N_ACTIONS:
            raise ValueError(f'the head has {k} outputs: {N_ACTIONS} (one per hinge) are needed')
        if activation not in ('relu', 'elu', 'tanh'):
            raise ValueError(f"activation must be 'relu', 'elu' or 'tanh', got {activation!r}")
        if out_activation not in (None, 'none', 'tanh'):
            raise ValueError(f"out_activation must be None or 'tanh', got {out_activation!r}")
        self.activation, self.out_activation = activation, out_activation or 'none'
        self.feed_last_action = bool(feed_last_action)
        self.height_scan = height_scan
        self.in_obs = _scan_split(self.in_dim, self.feed_last_action, height_scan, 'the cell')
        self.widths = [w.shape[1] for w in self.head_weights]
        col = lambda v: None if v is None else np.array(np.broadcast_to(np.asarray(v, dtype=np.float32), (self.in_obs,)), dtype=np.float32)
        self.obs_shift, self.obs_scale = col(obs_shift), col(obs_scale)
        # the head as an MlpPolicy of its own: its packing, its float64 form
        self.head = MlpPolicy(self.head_weights, self.head_biases, activation=activation, out_activation=out_activation)
        self._device = {}

    @classmethod
    def from_torch(cls, cell, head, **kw):
        """From a ``torch.nn.GRUCell`` or a one-layer unidirectional ``torch.nn.GRU`` (its ``weight_ih_l0`` ...) and a head
        ``torch.nn.Sequential`` as ``MlpPolicy.from_torch`` takes it; anything else raises ``ValueError``."""
        import torch.nn as nn
        if isinstance(cell, nn.GRUCell):
            names = ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')
            has_bias = cell.bias
        elif isinstance(cell, nn.GRU):
            if cell.num_layers != 1 or cell.bidirectional or getattr(cell, 'proj_size', 0):
                raise ValueError(f'a one-layer unidirectional GRU is supported, got num_layers = {cell.num_layers}, bidirectional = {cell.bidirectional}')
            names = ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')
            has_bias = cell.bias
        else:
            raise ValueError(f'from_torch takes a torch.nn.GRUCell or torch.nn.GRU, got {type(cell).__name__}')
        H = cell.hidden_size
        get = lambda n: getattr(cell, n).detach().cpu().numpy()
        zeros = np.zeros(3 * H, dtype=np.float32)
        h = MlpPolicy.from_torch(head)
        return cls(get(names[0]).T, get(names[1]).T, get(names[2]) if has_bias else zeros, get(names[3]) if has_bias else zeros, h.weights, h.biases,
                   activation=h.activation, out_activation=h.out_activation, **kw)

    def _gates(self):
        """the six gate layers in the blob's order: (W [K, H], b [H]) of ir, hr, iz, hz, in, hn"""
        H = self.hidden
        out = []
        for g in range(3):
            sl = slice(g * H, (g + 1) * H)
            out += [(self.w_ih[:, sl], self.b_ih[sl]), (self.w_hh[:, sl], self.b_hh[sl])]
        return out

    def blob_floats(self):
        return sum(_np(w.shape[1]) * (_kp(w.shape[0]) + 1) for w, _ in self._gates()) + self.head.blob_floats()

    def pack(self):
        """The padded blob (float32 numpy): the gate layers ``W_ir b_ir | W_hr b_hr | W_iz b_iz | W_hz b_hz | W_in b_in | W_hn b_hn`` in
        ``MlpPolicy.pack``'s per-layer layout, then the head's layers; zeros in the padding."""
        gates = self._gates()
        cell = MlpPolicy.__new__(MlpPolicy)   # (its pack() reads the two lists alone)
        cell.weights, cell.biases = [np.ascontiguousarray(w) for w, _ in gates], [np.ascontiguousarray(b) for _, b in gates]
        return np.ascontiguousarray(np.concatenate([cell.pack(), self.head.pack()]))

    def reference(self, x, h):
        """float64 evaluation over rows ``x [n, in_dim]`` (shift / scale applied to the first ``in_obs`` columns) and states ``h [n, H]``:
        ``(a [n, 12], h' [n, H])``."""
        x = np.array(x, dtype=np.float64).reshape(-1, self.in_dim)
        h = np.array(h, dtype=np.float64).reshape(-1, self.hidden)
        if self.obs_shift is not None:
            x[:, :self.in_obs] -= self.obs_shift.astype(np.float64)
        if self.obs_scale is not None:
            x[:, :self.in_obs] *= self.obs_scale.astype(np.float64)
        H = self.hidden
        gi = x @ self.w_ih.astype(np.float64) + self.b_ih.astype(np.float64)
        gh = h @ self.w_hh.astype(np.float64) + self.b_hh.astype(np.float64)
        r = sig64(gi[:, :H] + gh[:, :H])
        z = sig64(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        hn = n + z * (h - n)
        return self.head.reference(hn), hn

    # -- the two C blocks, with the blob on `device`: (GqPolicyMlp - the loop, the input row, the head -, GqPolicyGru)
    def _struct(self, device, rows_given=False):
        import ctypes as C

        from .cabi import GqPolicyGru, GqPolicyMlp
        blob, shift, scale, in_obs = _device_tables(self, device, rows_given)
        m = GqPolicyMlp(struct_size=C.sizeof(GqPolicyMlp), n_layers=len(self.widths), in_obs=in_obs, feed_last_action=int(self.feed_last_action),
                        activation=GQ_ACT[self.activation], out_activation=GQ_ACT[self.out_activation], decimation=1, blob=None, blob_floats=0,
                        obs_shift=None if shift is None else shift.data_ptr(), obs_scale=None if scale is None else scale.data_ptr())
        m.width = (C.c_int32 * 4)(*(self.widths + [0] * (4 - len(self.widths))))
        g = GqPolicyGru(struct_size=C.sizeof(GqPolicyGru), hidden=self.hidden, blob=blob.data_ptr(), blob_floats=blob.numel(), hidden_state=None, hidden_seq=None)
        return m, g
