"""Recognition training step, the body of the reference's ``train()`` loop (ocrs_models/train_rec.py:107-153):
bf16 autocast forward + CTC loss, accuracy stats, NaN guard, backward, clip_grad_norm_(4.0), Adam step -- and the validation loop
``test()`` (ocrs_models/train_rec.py:163-217): eval-mode forward, CTC loss, greedy decode + character error rate."""
from __future__ import annotations

import math

import torch

from .checkpoint import load_checkpoint, save_checkpoint  # noqa: F401  (shared with train_detection, train_rec.py:9)
from .losses import CTCLoss
from .optim import Adam, clip_grad_norm_
from .text import DeviceRecognitionAccuracyStats, RecognitionAccuracyStats

NAN_LOSS_MESSAGE = "Training produced invalid loss. Check input and target lengths are compatible with CTC loss"


def make_stats(stats: str = "host"):
    """"host": RecognitionAccuracyStats (edit distances in Python); "device": DeviceRecognitionAccuracyStats (everything on the GPU)."""
    if stats == "host":
        return RecognitionAccuracyStats()
    if stats == "device":
        return DeviceRecognitionAccuracyStats()
    raise ValueError(f'stats must be "host" or "device", not {stats!r}')


def make_optimizer(model, lr: float = 1e-3) -> Adam:
    return Adam(model.parameters(), lr=lr)  # train_rec.py:381-382


def make_scheduler(optimizer) -> torch.optim.lr_scheduler.ReduceLROnPlateau:
    """train_rec.py:383-385: stepped once per epoch on the validation loss."""
    return torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, factor=0.1, patience=3)


def train_step(model, optimizer, batch: dict, device, stats: RecognitionAccuracyStats | None = None, loss_fn=None, check_nan: bool = True,
               max_norm: float = 4.0):
    """One iteration of train_rec.py:107-151.  Returns (loss, grad_norm) as device scalars."""
    loss_fn = loss_fn or CTCLoss()
    # the model emits W/4 + 1 steps but only the first W/4 count for the loss (train_rec.py:110)
    input_lengths = batch["image_width"].div(4, rounding_mode="floor")
    img = batch["image"].to(device, non_blocking=True)
    text_seq = batch["text_seq"].to(device, non_blocking=True)
    target_lengths = batch["text_len"]
    optimizer.zero_grad()
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        pred_seq = model(img)
        batch_loss = loss_fn(pred_seq, text_seq, input_lengths, target_lengths)
    finish_stats = None
    if getattr(stats, "device_resident", False):  # the whole update is queued here, on the targets already uploaded for the loss
        finish_stats = stats.update_async(text_seq, target_lengths, pred_seq.detach(), input_lengths)
    elif stats is not None:  # device part now, host part (edit distances) after the backward pass has been queued
        finish_stats = stats.update_async(batch["text_seq"], target_lengths.tolist(), pred_seq.detach(), input_lengths.tolist())
    if check_nan and math.isnan(batch_loss.item()):
        raise Exception(NAN_LOSS_MESSAGE)
    batch_loss.backward()
    grad_norm = clip_grad_norm_(model.parameters(), max_norm=max_norm)
    optimizer.step()
    if finish_stats is not None:
        finish_stats()
    return batch_loss.detach(), grad_norm


def train(epoch: int, device, dataloader, model, optimizer, stats: str = "host"):
    """Epoch loop with the reference's signature and return value (train_rec.py:85-160).

    ``stats="device"`` (extension; the default is the reference's behaviour): the accuracy stats are a DeviceRecognitionAccuracyStats and the
    per-step ``isnan(loss.item())`` becomes a device-side count of non-finite losses that is read, with the two means, in ONE host
    synchronisation at the end of the epoch; the reference's exception is raised then.
    """
    model.train()
    on_device = stats == "device"
    stats = make_stats(stats)
    loss_fn = CTCLoss()
    mean_loss = torch.zeros((), device=device)
    total_norm = torch.zeros((), device=device)
    n = 0
    if on_device:
        bad = torch.zeros((), device=device)
        for batch in dataloader:
            loss, gn = train_step(model, optimizer, batch, device, stats, loss_fn, check_nan=False)
            mean_loss += loss
            total_norm += gn
            bad += (~torch.isfinite(loss)).float()
            n += 1
        loss_sum, norm_sum, nbad = torch.stack([mean_loss, total_norm, bad]).tolist()  # the epoch's one host synchronisation
        if nbad > 0:
            raise Exception(NAN_LOSS_MESSAGE)
        print(f"Mean grad norm {norm_sum / max(n, 1)}")
        return loss_sum / max(n, 1), stats
    for batch in dataloader:
        loss, gn = train_step(model, optimizer, batch, device, stats, loss_fn)
        mean_loss += loss
        total_norm += gn
        n += 1
    print(f"Mean grad norm {float(total_norm.item()) / max(n, 1)}")
    return float(mean_loss.item()) / max(n, 1), stats


def test(device, dataloader, model, preview: int = 10, stats: str = "host"):
    """Validation loop with the reference's signature and return value (mean loss, RecognitionAccuracyStats) (train_rec.py:163-217).
    ``stats="device"`` (extension): DeviceRecognitionAccuracyStats on the uploaded targets; with ``preview=0`` the mean loss read at the end is
    the epoch's only host synchronisation.

    Like the reference's, it runs outside autocast (fp32 kernels) and in eval mode; the first batch's first ``preview`` predictions are
    printed next to their targets.
    """
    from .text import DEFAULT_ALPHABET, ctc_greedy_decode_text, decode_text

    model.eval()
    on_device = stats == "device"
    stats = make_stats(stats)
    loss_fn = CTCLoss()
    mean_loss = torch.zeros((), device=device)
    n = 0
    with torch.no_grad():
        for batch_idx, batch in enumerate(dataloader):
            input_lengths = batch["image_width"].div(4, rounding_mode="floor")
            img = batch["image"].to(device, non_blocking=True)
            text_seq = batch["text_seq"].to(device, non_blocking=True)
            target_lengths = batch["text_len"]
            pred_seq = model(img)
            if on_device:
                stats.update(text_seq, target_lengths, pred_seq, input_lengths)
            else:
                stats.update(batch["text_seq"], target_lengths.tolist(), pred_seq, input_lengths.tolist())
            if batch_idx == 0 and preview:
                amax = pred_seq[:, : min(preview, pred_seq.shape[1]), :].argmax(-1).T.cpu()
                for i in range(amax.shape[0]):
                    target_text = decode_text(batch["text_seq"][i], list(DEFAULT_ALPHABET))
                    pred_text = ctc_greedy_decode_text(amax[i][: int(input_lengths[i])], list(DEFAULT_ALPHABET))
                    print(f'Sample test prediction "{pred_text}" target "{target_text}"')
            mean_loss += loss_fn(pred_seq, text_seq, input_lengths, target_lengths)
            n += 1
    return float(mean_loss.item()) / max(n, 1), stats
