"""Recognition training step, the body of the reference's ``train()`` loop (ocrs_models/train_rec.py:107-153):
bf16 autocast forward + CTC loss, accuracy stats, NaN guard, backward, clip_grad_norm_(4.0), Adam step -- and the validation loop
``test()`` (ocrs_models/train_rec.py:163-217): eval-mode forward, CTC loss, greedy decode + character error rate; and its ``main()``
(train_rec.py:307-462) on the device-resident dataset of ``ocrs_models_amd.datasets``:
``python -m ocrs_models_amd.train_rec hiertext DATA_DIR``.  No experiment tracking here."""
from __future__ import annotations

import math
import os
from argparse import ArgumentParser, BooleanOptionalAction

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


CHECKPOINT_FILE = "text-rec-checkpoint.pt"


def main(argv=None):
    """The reference's training script (train_rec.py:307-462) without wandb: same arguments, seed, validation-size rule, print lines,
    scheduler and checkpoint file.  ``--stats device`` (extension) keeps the accuracy statistics on the GPU.  Started by a launcher with
    WORLD_SIZE > 1 it is one rank of a data-parallel run: the model is wrapped in ``ddp.DistributedDataParallel``, the training batches
    come from a ``WidthBucketedDistributedSampler`` over the dataset's widths, every rank validates (the scheduler steps on the validation
    loss everywhere), and rank 0 alone prints and saves."""
    from .datasets import DeviceLineLoader, HierTextRecognition
    from .recognition import RecognitionModel
    from .text import DEFAULT_ALPHABET

    parser = ArgumentParser(description="Train text recognition model.")
    parser.add_argument("dataset_type", type=str, choices=["hiertext"])
    parser.add_argument("data_dir")
    parser.add_argument("--augment", default=True, action=BooleanOptionalAction, help="Enable data augmentations")
    parser.add_argument("--batch-size", type=int, default=20)
    parser.add_argument("--checkpoint", type=str, help="Model checkpoint to load")
    parser.add_argument("--export", type=str, help="Export model to ONNX format")
    parser.add_argument("--lr", type=float, help="Initial learning rate")
    parser.add_argument("--max-epochs", type=int, help="Maximum number of epochs to train for")
    parser.add_argument("--max-images", type=int, help="Maximum number of items to train on")
    parser.add_argument("--validate-only", action="store_true", help="Run validation on an exiting model")
    parser.add_argument("--stats", choices=["host", "device"], default="host", help="Where the accuracy statistics are computed")
    args = parser.parse_args(argv)

    if not torch.cuda.is_available():
        raise RuntimeError("ocrs_models_amd.train_rec runs on MI355X only (no CPU path)")
    torch.manual_seed(1234)

    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    distributed = world > 1
    if distributed:
        import torch.distributed as dist

        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)))
        if not dist.is_initialized():
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", torch.cuda.current_device()))
    device = torch.device("cuda", torch.cuda.current_device())
    say = print if rank == 0 else (lambda *a, **k: None)

    max_images = args.max_images
    validation_max_images = max(10, int(max_images * 0.1)) if max_images else None
    if distributed and rank != 0:
        dist.barrier()  # rank 0 writes the lines files and the crop cache alone; the others then only read them
    train_dataset = HierTextRecognition(args.data_dir, train=True, max_images=max_images, augment=args.augment, device=device)
    train_sampler = None
    if distributed:
        from .sampler import WidthBucketedDistributedSampler

        train_sampler = WidthBucketedDistributedSampler(train_dataset.widths, args.batch_size, rank=rank, world_size=world, seed=1234)
        train_dataloader = DeviceLineLoader(train_dataset, batch_sampler=train_sampler)
    else:
        train_dataloader = DeviceLineLoader(train_dataset, batch_size=args.batch_size, shuffle=True)
    val_dataset = HierTextRecognition(args.data_dir, train=False, max_images=validation_max_images, device=device)
    val_dataloader = DeviceLineLoader(val_dataset, batch_size=args.batch_size, shuffle=True)
    if distributed and rank == 0:
        dist.barrier()

    model = RecognitionModel(alphabet=DEFAULT_ALPHABET).to(device)
    optimizer = make_optimizer(model, lr=args.lr or 1e-3)  # 1e-3 is the Adam default
    scheduler = make_scheduler(optimizer)
    total_params = sum(p.numel() for p in model.parameters() if p.requires_grad)
    say(f"Model param count {total_params}")

    epoch = 0
    if args.checkpoint:
        checkpoint = load_checkpoint(args.checkpoint, model, optimizer, device)
        epoch = checkpoint["epoch"]

    if args.export:
        from .export import export_onnx

        test_batch = next(iter(val_dataloader))
        if rank == 0:
            export_onnx(model, args.export, test_batch["image"].to(device))
        return

    if args.validate_only:
        val_loss, val_stats = test(device, val_dataloader, model, stats=args.stats)
        say(f"Validation loss {val_loss} char error rate {val_stats.char_error_rate()}")
        return

    net = model
    if distributed:
        from .ddp import DistributedDataParallel

        net = DistributedDataParallel(model)

    while args.max_epochs is None or epoch < args.max_epochs:
        if train_sampler is not None:
            train_sampler.set_epoch(epoch)
        train_loss, train_stats = train(epoch, device, train_dataloader, net, optimizer, stats=args.stats)
        say(f"Epoch {epoch} train loss {train_loss} char error rate {train_stats.char_error_rate()}")
        val_loss, val_stats = test(device, val_dataloader, model, stats=args.stats)  # (every rank: the scheduler steps on it everywhere)
        say(f"Epoch {epoch} validation loss {val_loss} char error rate {val_stats.char_error_rate()}")
        scheduler.step(val_loss)
        say(f"Current learning rate {scheduler.get_last_lr()}")
        if rank == 0:
            save_checkpoint(CHECKPOINT_FILE, model, optimizer, epoch=epoch)
        epoch += 1


if __name__ == "__main__":
    main()
