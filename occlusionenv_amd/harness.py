"""Harness counterparts of the reference's callers of the hot path -- the loops that drive
``step()`` and consume its outputs (the PPO learner is ``ppo.BatchedPPO``, the frozen encoder ``encoder.FrozenEncoder``):

  * ``gradient_ascent``  -- demo.py:80-114 / iterator.py:112-138: ``action = nn.Parameter(zeros(2))``,
    ``reward.backward()``, skip NaN gradients, ``action += lr * action.grad``.
  * ``collect_rollout``  -- trainRL.py:189-229 + PPO.py:152-164 in batched form: T steps of a policy over N envs,
    one rollout record per env-step (256 pooled features, action, logprob, reward, done = 1044 B) and one
    all-gather of the records per step when torch.distributed is initialised (rollout.py).
  * ``evaluate_segmentation`` -- the measuring half of pretrainer.py:176-189 (``val``) against the live environment
    instead of a stored dataset: the predicted occlusion map of a FullNetwork checkpoint against the occlusion image
    every step renders anyway.
  * ``finetune_segmentation`` -- the learning half of the same loop (pretrainer.py:91,120-141): every step's occlusion image is
    the target of one AdamW step on the segmentation head (``seghead.SegmentationHead``), the encoder frozen.
  * ``train_predictor`` -- train_predict.py:38-69 on the batched env: random actions, the engine's action gradient as the
    target of the gradient predictor, MSE and AdamW on the dense encoder and its head (``enctrain.TrainableEncoder``).
  * ``validate_pretrained`` -- pretrainer.py:162-204 (``val``) itself, on a stored dataset: Loss / Dice / MSE / Accuracy /
    IoU as the means of the per-batch values.
  * ``pretrain_epoch`` -- pretrainer.py:112-159 (``train``) on a stored dataset: the summed segmentation and gradient loss
    back-propagated through decoder, skips and encoder at once (``fullnet.TrainableFullNetwork``, or
    ``sepfullnet.TrainableSeparableFullNetwork`` for the separable network the agent runs), AdamW.  ``batch_stats=True``:
    BatchNorm in train mode as in the reference (batch statistics, running averages updated); the default keeps the running
    statistics.  ``native_optimizer=True``: ``netoptim.PackedAdamW``, the AdamW step in packed order in one native launch.
  * ``pretrain`` -- pretrainer.py:209-259 (``PreTrainer.run``): per epoch ``pretrain_epoch``, ``validate_pretrained`` on the
    trained network, one step of the cosine schedule; the state dict of the best validation IoU is kept.
  * ``evaluate_controllers`` -- test.py:92-255 / iterator.py:104-204, the experiment itself: the number of steps until
    ``finished`` for the raw gradient, a random walk, the pretrained network's predicted gradient and the PPO agent
    (``GradientAscent``, ``RandomWalk``, ``PredictedGradient``, ``Agent``) on the same scenes, all envs at once with the
    episode bookkeeping on the device; ``write_iterations`` writes the reference's ``iterations_*.txt``,
    ``summarise_iterations`` the means, medians and paired differences.  They live in ``episodes.py``.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch

from . import rollout
from .episodes import (Agent, GradientAscent, PredictedGradient, RandomWalk, controller_generators,  # noqa: F401
                       evaluate_controllers, summarise_iterations, write_iterations)


def gradient_ascent(env, steps: int = 20, lr: float = 0.01, reset_kwargs: Optional[dict] = None):
    """Gradient ascent on the viewpoint action through env.step (single OcclusionEnv).  Returns the list of
    (reward, full_reward, done) per step and the final action."""
    env.reset(**(reset_kwargs or {}))
    action = torch.nn.Parameter(torch.zeros(2, device=env.device))
    log = []
    for _ in range(steps):
        if action.grad is not None:
            action.grad = None
        obs, reward, done, info = env.step(action)
        reward.backward()
        if torch.isnan(action.grad).any():  # demo.py:87-89
            continue
        with torch.no_grad():
            action += lr * action.grad
        log.append((float(reward), float(info["full_reward"]), bool(done)))
        if done:
            break
    return log, action.detach()


def gaussian_policy(std: float = 0.6) -> Callable:
    """Stand-in for ActorCritic.act (PPO.py:62-80): diagonal Gaussian around a linear read-out of the pooled
    features; returns (action, logprob).  The reference's actor is the frozen FullNetwork encoder + a linear head:
    ``encoder.FrozenEncoder`` and ``ppo.BatchedPPO.from_fullnetwork``."""
    w = None

    def act(features: torch.Tensor):
        nonlocal w
        if w is None:
            g = torch.Generator(device="cpu").manual_seed(0)
            w = (torch.randn(256, 2, generator=g) * 0.05).to(features.device)
        mean = features @ w
        eps = torch.randn_like(mean)
        action = mean + std * eps
        logprob = (-0.5 * eps.pow(2) - torch.log(torch.tensor(std, device=mean.device)) - 0.9189385).sum(1)
        return action, logprob

    return act


def collect_rollout(venv, T: int = 50, policy: Optional[Callable] = None, with_grad: bool = True):
    """T batched steps.  Returns dict(records (T, world*N, 261), action_grads (T, N, 2) or None, obs)."""
    policy = policy or gaussian_policy()
    obs = venv.reset()[:, 0]
    recs, grads = [], []
    for _ in range(T):
        feats = rollout.pooled_features(obs)
        action, logprob = policy(feats)
        action = action.detach().requires_grad_(with_grad)
        obs, rewards, dones, infos = venv.step(action)
        if with_grad:
            rewards.sum().backward()  # train_predict.py:52
            grads.append(action.grad.detach().clone())
        rec = rollout.pack_records(obs, action, logprob, rewards, dones)
        recs.append(rollout.all_gather_records(rec))
    return dict(records=torch.stack(recs), action_grads=torch.stack(grads) if grads else None, obs=obs)


@torch.no_grad()
def evaluate_segmentation(venv, enc, steps: int, policy: Optional[Callable] = None) -> dict:
    """``steps`` batched steps of ``venv``; every step's observation goes through ``enc.forward_full`` and the predicted
    occlusion map is judged against the step's own occlusion image, the alpha channel of ``full_state`` (what
    dataset_io.py writes as the pretrainer's target), as pretrainer.py:133-141 judges it: both thresholded at 0.5, counts
    summed over everything seen.  ``policy(pooled) -> (action, logprob)`` chooses the actions (default: zeros).  Returns
    accuracy and IoU in percent, as the reference prints them, and the raw counts; one host sync, at the end."""
    obs = venv.reset()
    n = int(obs.shape[0])
    totals = torch.zeros(3, dtype=torch.int64, device=obs.device)
    pixels = 0
    action = torch.zeros(n, 2, device=obs.device)
    for _ in range(int(steps)):
        obs, _rewards, _dones, infos = venv.step(action)
        obs = obs[:, 0] if obs.dim() == 5 else obs
        occl = torch.cat([infos[i]["full_state"] for i in range(n)])[..., 3]
        pooled, segm, _grad = enc.forward_full(obs)
        m = enc.occlusion_metrics(segm, occl)
        totals += torch.stack([m["correct"].sum(), m["intersection"].sum(), m["union"].sum()])
        pixels += occl.numel()
        if policy is not None:
            action = policy(pooled)[0].detach()
    correct, inter, union = (int(v) for v in totals.tolist())
    return dict(accuracy=100.0 * correct / pixels if pixels else float("nan"),
                iou=100.0 * inter / union if union else float("nan"), correct=correct, intersection=inter, union=union,
                pixels=pixels)


def finetune_segmentation(venv, enc_or_head, steps: int, lr: float = 1e-3, weight_decay: float = 1e-5, use_dice: bool = True,
                          policy: Optional[Callable] = None) -> dict:
    """The loop of ``evaluate_segmentation`` with a learning step inside: every step renders, takes the engine's occlusion
    map (the alpha channel of ``full_state``) as the target, applies ``binary_dice_loss`` (``use_dice``) or
    ``binary_cross_entropy`` to ``head(obs)``, runs ``backward`` and one ``torch.optim.AdamW`` step (the optimizer of
    pretrainer.py:91) on the head's parameters.  ``enc_or_head``: a ``SegmentationHead``, or a ``FrozenEncoder`` with a
    decoder, from which one is made.  The decoder's BatchNorm keeps its running statistics (``seghead``).  Returns ``head``,
    the per-step ``losses`` and the per-step ``accuracy`` / ``iou`` in percent of the prediction the step learned from
    (``segmentation.seg_criterion``'s counts), as lists of floats; one host sync, at the end."""
    from . import segmentation
    from .seghead import SegmentationHead

    head = enc_or_head if isinstance(enc_or_head, SegmentationHead) else SegmentationHead.from_encoder(enc_or_head)
    opt = torch.optim.AdamW(head.parameters(), lr=lr, weight_decay=weight_decay)
    obs = venv.reset()
    n = int(obs.shape[0])
    action = torch.zeros(n, 2, device=obs.device)
    rows = []
    for _ in range(int(steps)):
        obs, _rewards, _dones, infos = venv.step(action)
        obs = obs[:, 0] if obs.dim() == 5 else obs
        occl = torch.cat([infos[i]["full_state"] for i in range(n)])[..., 3]
        opt.zero_grad(set_to_none=True)
        pooled, segm = head(obs, return_features=True)
        loss = segmentation.binary_dice_loss(segm, occl) if use_dice else segmentation.binary_cross_entropy(segm, occl)
        loss.backward()
        opt.step()
        c = segmentation.seg_criterion(segm, occl)
        correct, inter, union = c["correct"].sum().double(), c["intersection"].sum().double(), c["union"].sum().double()
        rows.append(torch.stack([loss.detach().double(), 100.0 * correct / float(occl.numel()), 100.0 * inter / union]))
        if policy is not None:
            action = policy(pooled)[0].detach()
    host = torch.stack(rows).cpu().tolist() if rows else []
    return dict(head=head, losses=[r[0] for r in host], accuracy=[r[1] for r in host], iou=[r[2] for r in host], steps=len(host))


def train_predictor(venv, enc_or_net, steps: int, lr: float = 1e-4, weight_decay: float = 1e-2, reset_every: int = 10):
    """train_predict.py:38-69 on the batched env: every ``reset_every`` steps (the reference's episode length) the envs are
    reset; every step draws ``action = randn(N, 2)``, steps, takes ``rewards.sum().backward()`` for the engine's action
    gradient, skips the step if that gradient has a NaN (line 53), normalises it per env as on line 58
    (``g / sqrt(sum g^2 + 1e-7)``) and applies ``F.mse_loss(net.predict_grad(obs), target)``, ``backward`` and one
    ``torch.optim.AdamW`` step (``weight_decay``: torch's default, as in the reference) to the encoder and its head.
    ``enc_or_net``: an ``enctrain.TrainableEncoder`` or a ``septrain.TrainableSeparableEncoder``, or a ``FrozenEncoder`` with
    a grad head, from which the one for its form (dense or separable) is made.  BatchNorm keeps its running statistics
    (``enctrain``).  Returns ``net``, the per-step ``losses``
    of the steps that learned (floats) and ``skipped``, the number of NaN steps; one host sync per step, for the NaN test
    the reference makes there too."""
    from .enctrain import PooledFeatureNet, TrainableEncoder
    from .septrain import TrainableSeparableEncoder

    if isinstance(enc_or_net, PooledFeatureNet):
        net = enc_or_net
    elif getattr(enc_or_net, "separable", False):
        net = TrainableSeparableEncoder.from_encoder(enc_or_net)
    else:
        net = TrainableEncoder.from_encoder(enc_or_net)
    opt = torch.optim.AdamW(net.parameters(), lr=lr, weight_decay=weight_decay)
    losses, skipped = [], 0
    obs = None
    for i in range(int(steps)):
        if obs is None or (reset_every and i % int(reset_every) == 0):
            obs = venv.reset()
        n = int(obs.shape[0])
        action = torch.randn(n, 2, device=obs.device).requires_grad_(True)
        opt.zero_grad(set_to_none=True)
        obs, rewards, _dones, _infos = venv.step(action)
        rewards.sum().backward()
        if bool(torch.isnan(action.grad).any()):
            skipped += 1
            continue
        frame = (obs[:, 0] if obs.dim() == 5 else obs).detach()
        target = action.grad / torch.sqrt((action.grad ** 2).sum(dim=1, keepdim=True) + 1e-7)
        loss = torch.nn.functional.mse_loss(net.predict_grad(frame), target.detach())
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    host = torch.stack(losses).cpu().tolist() if losses else []
    return dict(net=net, losses=host, skipped=skipped, steps=len(host))


def _pretrain_net(net_or_enc, batch_stats: bool):
    """The joint network of ``pretrain_epoch`` / ``pretrain``: ``net_or_enc`` itself, or the one for the encoder's form."""
    from .fullnet import JointNet, TrainableFullNetwork
    from .sepfullnet import TrainableSeparableFullNetwork

    if isinstance(net_or_enc, JointNet):
        net = net_or_enc
    elif getattr(net_or_enc, "separable", False):
        net = TrainableSeparableFullNetwork.from_encoder(net_or_enc, batch_stats=batch_stats)
    else:
        net = TrainableFullNetwork.from_encoder(net_or_enc, batch_stats=batch_stats)
    if not net.has_grad_head or net.enc.preset != "ppo":
        raise ValueError("pretrain_epoch needs a FullNetwork checkpoint (preset 'ppo') with its gradPredictor head")
    return net


def _pretrain_optimizer(net, lr: float, weight_decay: float, native: bool):
    """pretrainer.py:91's AdamW for ``net``: ``netoptim.PackedAdamW`` (``native``) or ``torch.optim.AdamW`` on its parameters."""
    if native:
        from .netoptim import PackedAdamW

        return PackedAdamW(net, lr=lr, weight_decay=weight_decay)
    if net._resident is not None:
        raise ValueError("this net is packed-resident (netoptim.PackedAdamW): pass its optimizer or native_optimizer=True")
    return torch.optim.AdamW(net.parameters(), lr=lr, weight_decay=weight_decay)


def pretrain_epoch(net_or_enc, batches, use_dice: bool = True, use_l1: bool = False, lr: float = 1e-3, weight_decay: float = 1e-5,
                   optimizer=None, batch_stats: bool = False, native_optimizer: bool = False) -> dict:
    """One epoch of ``PreTrainer.train()`` (pretrainer.py:112-159) on the device: ``batches`` is any iterable of
    ``(img, occlusion, grad, _)`` as for ``validate_pretrained``.  Every batch goes through ``net(img)``
    (``fullnet.TrainableFullNetwork`` or ``sepfullnet.TrainableSeparableFullNetwork``: one native forward of encoder, decoder
    and classifier, the grad head in torch), takes
    ``segmentation.binary_dice_loss`` (``use_dice``) or ``binary_cross_entropy`` of the map plus ``nn.MSELoss()`` or
    ``nn.SmoothL1Loss(beta=0.01)`` (``use_l1``) of the gradient prediction, runs ``backward`` (one native joint backward)
    and one ``torch.optim.AdamW`` step (pretrainer.py:91; ``optimizer``: one to carry over epochs, made here when None;
    ``native_optimizer=True`` makes a ``netoptim.PackedAdamW`` instead, after which the net is packed-resident and only that
    optimizer trains it).
    ``net_or_enc``: a ``TrainableFullNetwork`` or a ``TrainableSeparableFullNetwork``, or a "ppo" ``FrozenEncoder`` with decoder
    and grad head, from which the one for its form (dense or separable) is made, with ``batch_stats`` passed on:
    False, BatchNorm keeps its running statistics; True, it runs in train mode as the reference's does (``fullnet``), each
    batch needing ``N (S / 32)^2 >= 2``.  A net that is passed in keeps its own setting.  Returned are ``net``, ``optimizer`` and the five numbers
    the reference prints, computed its way: ``loss``, ``segm_loss``, ``grad_loss`` = the mean over batches of the per-batch
    losses, ``accuracy`` and ``iou`` = the mean over batches of the per-batch ratios x 100 of the prediction the step learned
    from (``segmentation.seg_criterion``'s counts); also the pooled ``correct``, ``intersection``, ``union``, ``pixels``
    and ``batches``.  One host sync, at the end."""
    from . import segmentation

    net = _pretrain_net(net_or_enc, batch_stats)
    opt = optimizer if optimizer is not None else _pretrain_optimizer(net, lr, weight_decay, native_optimizer)
    dev = net.enc.device
    rows, totals, pixels = [], None, 0
    for img, occlusion, grad, *_ in batches:
        img, occlusion, grad = img.to(dev), occlusion.to(dev), grad.to(dev, torch.float32)
        opt.zero_grad(set_to_none=True)
        _pooled, segm, grad_pred = net(img)
        segm_loss = segmentation.binary_dice_loss(segm, occlusion) if use_dice else segmentation.binary_cross_entropy(segm, occlusion)
        grad_loss = (torch.nn.functional.smooth_l1_loss(grad_pred, grad, beta=0.01) if use_l1
                     else torch.nn.functional.mse_loss(grad_pred, grad))
        loss = grad_loss + segm_loss
        loss.backward()
        opt.step()
        c = segmentation.seg_criterion(segm, occlusion)
        t = torch.stack([c["correct"].sum(), c["intersection"].sum(), c["union"].sum()])
        td = t.double()
        rows.append(torch.stack([loss.detach().double(), segm_loss.detach().double(), grad_loss.detach().double(),
                                 td[0] / float(segm.numel()), td[1] / td[2]]))
        totals = t if totals is None else totals + t
        pixels += segm.numel()
    if not rows:
        raise ValueError("pretrain_epoch: no batches")
    host = torch.cat([torch.stack(rows).mean(0), totals.double()]).cpu().tolist()
    loss, segm_loss, grad_loss, acc, iou = host[:5]
    correct, inter, union = (int(x) for x in host[5:])
    return dict(net=net, optimizer=opt, loss=loss, segm_loss=segm_loss, grad_loss=grad_loss, accuracy=100.0 * acc, iou=100.0 * iou,
                correct=correct, intersection=inter, union=union, pixels=pixels, batches=len(rows))


def pretrain(net_or_enc, train_batches, val_batches, epochs: int, use_dice: bool = True, use_l1: bool = False, lr: float = 1e-3,
             weight_decay: float = 1e-5, batch_stats: bool = False, native_optimizer: bool = True) -> dict:
    """``PreTrainer.run()`` (pretrainer.py:209-259) on the device: ``epochs`` times ``pretrain_epoch`` on ``train_batches``,
    ``validate_pretrained`` of the trained network (``enc.with_state(net.state_dict())``) on ``val_batches``, and one step of
    ``CosineAnnealingLR(optimizer, epochs, eta_min=0.1 * lr)``; the state dict after the epoch with the best validation IoU
    so far is kept (a copy, as the reference saves a file).  ``train_batches`` / ``val_batches``: a callable returning the
    epoch's iterable of batches, or a re-iterable (a list, a DataLoader), so that every epoch sees its batches again.
    ``native_optimizer``: ``netoptim.PackedAdamW`` (the default here) or ``torch.optim.AdamW``; the other arguments are
    ``pretrain_epoch``'s.  Returns ``net``, ``optimizer``, ``rows`` (per epoch ``epoch``, ``lr`` = the rate the epoch trained
    with, ``train`` and ``val`` = the two dicts of numbers), ``best_epoch``, ``best_iou`` and ``best_state``.  A validation
    IoU of nan (a batch with an empty union) never counts as best; without any other, the first epoch's state is returned."""
    if int(epochs) < 1:
        raise ValueError("pretrain: epochs must be >= 1")

    def each(batches):
        return batches() if callable(batches) else batches

    net = _pretrain_net(net_or_enc, batch_stats)
    opt = _pretrain_optimizer(net, lr, weight_decay, native_optimizer)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, int(epochs), eta_min=0.1 * lr)
    rows, best_iou, best_epoch, best_state = [], float("-inf"), None, None
    for epoch in range(int(epochs)):
        trained = float(opt.param_groups[0]["lr"])
        res = pretrain_epoch(net, each(train_batches), use_dice=use_dice, use_l1=use_l1, optimizer=opt)
        state = {k: v.detach().clone() for k, v in net.state_dict().items()}
        val = validate_pretrained(net.enc.with_state(state), each(val_batches), use_dice=use_dice, use_l1=use_l1)
        sched.step()
        rows.append(dict(epoch=epoch, lr=trained, train={k: v for k, v in res.items() if k not in ("net", "optimizer")}, val=val))
        if val["iou"] > best_iou or best_state is None:
            best_epoch, best_state = epoch, state
            best_iou = val["iou"] if val["iou"] == val["iou"] else best_iou
    return dict(net=net, optimizer=opt, rows=rows, best_epoch=best_epoch, best_iou=best_iou, best_state=best_state)


@torch.no_grad()
def validate_pretrained(enc, batches, use_dice: bool = True, use_l1: bool = False) -> dict:
    """``PreTrainer.val()`` (pretrainer.py:162-204) for a FullNetwork checkpoint loaded as ``enc`` (a ``FrozenEncoder``):
    ``batches`` is any iterable of ``(img, occlusion, grad, _)``, as ``dataset_io.OcclusionDataset`` behind a DataLoader
    yields them (host tensors are moved to the encoder's device).  Every batch goes through ``enc.forward_full`` and
    ``enc.validation_losses``; returned are the five numbers the reference prints and selects a checkpoint by, computed its
    way: ``loss``, ``segm_loss``, ``grad_loss`` = the mean over batches of the per-batch losses, ``accuracy`` and ``iou`` =
    the mean over batches of the per-batch ratios x 100 (a batch with an empty union contributes nan, as in the reference;
    ``evaluate_segmentation`` pools the counts instead).  Also the pooled counts ``correct``, ``intersection``, ``union``,
    ``pixels`` and ``batches``.  One host sync, at the end."""
    rows, totals, pixels = [], None, 0
    for img, occlusion, grad, *_ in batches:
        img, occlusion, grad = img.to(enc.device), occlusion.to(enc.device), grad.to(enc.device)
        _pooled, segm, grad_pred = enc.forward_full(img)
        v = enc.validation_losses(segm, grad_pred, occlusion, grad, use_dice=use_dice, use_l1=use_l1)
        rows.append(torch.stack([v[k].double() for k in ("loss", "segm_loss", "grad_loss", "accuracy", "iou")]))
        t = torch.stack([v["correct"].sum(), v["intersection"].sum(), v["union"].sum()])
        totals = t if totals is None else totals + t
        pixels += segm.numel()
    if not rows:
        raise ValueError("validate_pretrained: no batches")
    means = torch.stack(rows).mean(0)
    # one transfer: the counts are exact in f64 below 2^53
    host = torch.cat([means, totals.double()]).cpu().tolist()
    loss, segm_loss, grad_loss, acc, iou = host[:5]
    correct, inter, union = (int(x) for x in host[5:])
    return dict(loss=loss, segm_loss=segm_loss, grad_loss=grad_loss, accuracy=100.0 * acc, iou=100.0 * iou, correct=correct,
                intersection=inter, union=union, pixels=pixels, batches=len(rows))
