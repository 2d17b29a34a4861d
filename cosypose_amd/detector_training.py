"""The loop around the detector's training step, in the shape of training.train_loop.

Contract (cosypose/training/train_detector.py:206-314, maskrcnn_forward_loss.py):
  * h_maskrcnn: the five losses of the Mask R-CNN, weighted by cfg.rpn_box_reg_alpha, objectness_alpha, box_reg_alpha, classifier_alpha and
    mask_alpha and added in that order; each goes to the meter of its name.  Frames are the uint8 HWC tensors DetectionDataset collates (the
    reference's `.float() / 255` is Detector.losses' own first kernel); what arrives on the CPU is uploaded with non_blocking=True.
  * step (:256-275): zero_grad -> h_maskrcnn -> backward -> the total gradient norm (clip_grad_norm_(max_norm=inf): logged, never applied) ->
    SGD step -> the warm-up scheduler.  With detector_optim.FlatSGD norm, update and the repack of every layer are three launches on flat
    buffers, and the gradient averaging of a multi-rank run is one all-reduce of the flat gradient (train_engine.allreduce_gradients) in
    the place of the reference's DistributedDataParallel.
  * schedule (:223-236): training.LRSchedule, the state machine of the two chained torch schedulers, the resumed state included.
  * epoch end (:277-314): the StepLR; the validation losses under torch.no_grad() every cfg.val_epoch_interval epochs; the checkpoint
    {'state_dict', 'epoch'} by rank 0; the log dict's train_* / val_* / grad_norm / learning_rate entries go to on_epoch_end.
  * The reference saves no optimiser state: a resumed run restarts with empty momentum.  save_optimizer=True writes optimizer.pth.tar beside
    the checkpoint and a resumed run loads it, so an interrupted run continues bit for bit (with faithful_schedule=False; the faithful
    schedule restarts the warm-up, as the reference does).
Datasets, samplers, the evaluation during training (run_eval), log.txt and bokeh are out of scope: `batches` is any iterable of (images, targets).
"""
import pathlib
import warnings
from collections import defaultdict

import torch

from . import train_engine
from .training import LRSchedule, LazyMeters, _Mean, save_checkpoint

LOSSES = ('loss_rpn_box_reg', 'loss_objectness', 'loss_box_reg', 'loss_classifier', 'loss_mask')       # the reference's order of the weighted sum
ALPHAS = ('rpn_box_reg_alpha', 'objectness_alpha', 'box_reg_alpha', 'classifier_alpha', 'mask_alpha')


def _device_of(detector):
    params = detector.parameters()
    return next(iter(params)).device


def _cast(t, dev):
    t = torch.as_tensor(t)
    return t if t.device == dev else t.to(dev, non_blocking=True)


def _add(meters, names, values):
    """values: 1-D tensor; LazyMeters take device values without stopping the host, any other mapping of meters reads them now"""
    if hasattr(meters, 'defer'):
        meters.defer([(n,) for n in names], values)
    else:
        for n, v in zip(names, values.detach().tolist()):
            meters[n].add(v)


def h_maskrcnn(data, detector, meters, cfg, generator=None):
    """data = (images, targets): uint8 HWC frames and their {'boxes', 'labels', 'masks'} -> the weighted sum of the five losses, with autograd
    history when grad is enabled.  generator: the device torch.Generator the samplers draw their keys from."""
    images, targets = data
    dev = _device_of(detector)
    frames = [_cast(im, dev) for im in images]
    targets = [{k: _cast(v, dev) for k, v in t.items()} for t in targets]
    loss_dict = detector.losses(frames, targets, generator=generator)
    loss = None
    for name, alpha in zip(LOSSES, ALPHAS):
        term = getattr(cfg, alpha) * loss_dict[name]
        loss = term if loss is None else loss + term
    _add(meters, LOSSES, torch.stack([loss_dict[n].detach().reshape(()) for n in LOSSES]))
    return loss


def optimizer_path(save_dir):
    return pathlib.Path(save_dir) / 'optimizer.pth.tar'


def _generator(dev, seed, epoch, rank, stream=0):
    """equal (seed, epoch, rank) give equal sampler keys: a resumed epoch draws what the uninterrupted run drew.  stream 1: the validation's"""
    g = torch.Generator(device=dev)
    g.manual_seed((((int(seed) * 1000003 + int(epoch)) * 1000003 + int(rank)) * 2 + stream) % (2 ** 63 - 1))
    return g


def train_detector_loop(detector, cfg, batches, n_epochs, save_dir=None, start_epoch=0, optimizer=None, val_batches=None, on_epoch_end=None,
                        faithful_schedule=True, save_optimizer=False, seed=0):
    """Runs epochs [start_epoch, n_epochs) of the reference's detector training on `batches` (a callable epoch -> iterable of (images, targets),
    or a re-iterable).  cfg: lr, momentum, weight_decay, n_epochs_warmup, lr_epoch_decay, val_epoch_interval, the five *_alpha, and
    batches_per_epoch or epoch_size and batch_size (the warm-up's length; default: the length of the first epoch).  optimizer: anything with
    param_groups, zero_grad() and step() (default: detector.optimizer(...), a FlatSGD).  Returns {epoch: mean total loss}."""
    import torch.distributed as dist
    from .detector_optim import FlatSGD
    multi = dist.is_available() and dist.is_initialized()
    world, rank = (dist.get_world_size(), dist.get_rank()) if multi else (1, 0)
    if optimizer is None:
        optimizer = detector.optimizer(lr=cfg.lr, momentum=cfg.momentum, weight_decay=cfg.weight_decay)
    flat = isinstance(optimizer, FlatSGD)
    if world > 1 and not flat:
        raise ValueError(f'train_detector_loop: {world} ranks, but the optimizer is not a FlatSGD: the ranks would train independently '
                         '(the gradient averaging is one all-reduce of FlatSGD\'s flat gradient)')
    if start_epoch > 0 and faithful_schedule:
        warnings.warn('train_detector_loop: resuming with faithful_schedule=True reproduces the reference\'s resume behaviour (train_detector.py:229: the '
                      'warm-up LambdaLR is rebuilt on resume): the learning rate restarts at lr / n_warm_batches and never recovers; pass '
                      'faithful_schedule=False for the intended schedule')
    if save_optimizer and start_epoch > 0 and save_dir is not None and optimizer_path(save_dir).exists():
        optimizer.load_state_dict(torch.load(optimizer_path(save_dir), map_location='cpu'))
    bpe = getattr(cfg, 'batches_per_epoch', None)      # the reference's warm-up length: epoch_size // batch_size (train_detector.py:227)
    if bpe is None and getattr(cfg, 'epoch_size', None) and getattr(cfg, 'batch_size', None):
        bpe = cfg.epoch_size // cfg.batch_size
    dev = _device_of(detector)
    lazy = dev.type == 'cuda'
    new_meters = (lambda: LazyMeters(_Mean)) if lazy else (lambda: defaultdict(_Mean))
    history, schedule = {}, None
    for epoch in range(start_epoch, n_epochs):
        it = batches(epoch) if callable(batches) else batches
        items = list(it) if schedule is None and not hasattr(it, '__len__') else it
        if schedule is None:
            schedule = LRSchedule(cfg.lr, cfg.n_epochs_warmup, bpe or len(items), cfg.lr_epoch_decay, start_epoch=start_epoch, faithful=faithful_schedule)
        if hasattr(detector, 'train'):
            detector.train()
        meters, meters_val = new_meters(), new_meters()
        gen = _generator(dev, seed, epoch, rank)
        for b, sample in enumerate(items):
            schedule.apply(optimizer, epoch, b)
            optimizer.zero_grad()
            loss = h_maskrcnn(sample, detector, meters, cfg, generator=gen)
            loss.backward()
            if flat:
                if world > 1:
                    train_engine.allreduce_gradients(optimizer)      # collects detached .grad tensors first
                norm = optimizer.step()
            else:
                norm = torch.nn.utils.clip_grad_norm_(detector.parameters(), max_norm=float('inf'), norm_type=2)
                optimizer.step()
            _add(meters, ('loss_total', 'grad_norm'), torch.stack([loss.detach().reshape(()), torch.as_tensor(norm, device=loss.device).detach().reshape(()).to(loss.dtype)]))
            schedule.after_batch(epoch)
        schedule.after_epoch(epoch)
        if val_batches is not None and epoch % cfg.val_epoch_interval == 0:
            gen_val = _generator(dev, seed, epoch, rank, stream=1)
            with torch.no_grad():
                for sample in (val_batches(epoch) if callable(val_batches) else val_batches):
                    loss = h_maskrcnn(sample, detector, meters_val, cfg, generator=gen_val)
                    _add(meters_val, ('loss_total',), loss.detach().reshape(1))
        for m in (meters, meters_val):
            if hasattr(m, 'flush'):
                m.flush()
        history[epoch] = meters['loss_total'].mean
        if save_dir is not None and rank == 0:
            save_checkpoint(detector, epoch, save_dir)
            if save_optimizer:
                torch.save(optimizer.state_dict(), optimizer_path(save_dir))
        if on_epoch_end is not None:
            # learning_rate: what the reference logs here, the rate its schedulers have just left in the optimiser for the next step
            means = {'grad_norm': meters['grad_norm'].mean, 'learning_rate': schedule.current(epoch + 1, 0)}
            means.update({f'train_{k}': m.mean for k, m in meters.items()})
            means.update({f'val_{k}': m.mean for k, m in meters_val.items()})
            on_epoch_end(epoch, means)
    return history
