"""Layout training and validation, the bodies of the reference's ``train()`` / ``test()`` loops (ocrs_models/train_layout.py:15-183):
forward, weighted BCE-with-logits, backward, Adam step, accuracy statistics -- with the loss and the statistics kept on the device (one host
synchronisation per epoch instead of three per batch), and its ``main()`` (train_layout.py:186-319) on the device-resident dataset of
``ocrs_models_amd.datasets``: ``python -m ocrs_models_amd.train_layout DATA_DIR``.  No experiment tracking here."""
from __future__ import annotations

from argparse import ArgumentParser

import torch
from torch import nn

from ._lib import lib, ptr
from .checkpoint import load_checkpoint, save_checkpoint  # noqa: F401  (train_layout.py:12)
from .datasets import DeviceWebLayoutLoader, WebLayout
from .layout import LayoutModel, loss_workspace  # noqa: F401
from .optim import Adam

POS_WEIGHT = 10.0  # train_layout.py:94-97: an estimate of 7-9 % of the words being positive for each class


def f1_score(precision: float, recall: float) -> float:
    """F1 mean of precision and recall (train_layout.py:15-21)."""
    return 2 * (precision * recall) / (precision + recall)


def precision_recall(preds: torch.Tensor, targets: torch.Tensor) -> tuple[float, float]:
    """Precision and recall of boolean predictions (train_layout.py:24-35): int64 counts divided as fp32, 0 / 0 = NaN.  Synchronises
    (``.item()``), like the reference; the loops use ``LayoutAccuracyStats`` instead, which does not."""
    true_results = torch.logical_and(preds, targets).sum()
    precision = true_results / preds.sum()
    recall = true_results / targets.sum()
    return (precision.item(), recall.item())


def lr_scale_for_epoch(epoch: int) -> float:
    """Scale of the initial learning rate for an epoch, for ``LambdaLR`` (train_layout.py:174-183)."""
    warmup_epochs = 50
    if warmup_epochs > 0:
        return min((epoch + 1) / (warmup_epochs + 1), 1)
    return 1


def _loss_launch(pred, target, pred_is_prob, want_grad, counts):
    if not pred.is_cuda:
        raise RuntimeError("ocrs_models_amd.train_layout runs on MI355X only (no CPU path)")
    if pred.dim() != 3 or pred.shape[2] != 2 or tuple(target.shape) != tuple(pred.shape):
        raise RuntimeError(f"expected (N, W, 2) predictions and targets, got {tuple(pred.shape)} and {tuple(target.shape)}")
    pred = pred.detach().contiguous().float()
    target = target.contiguous().float()
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    dlog = torch.empty_like(pred) if want_grad else None
    lib().layout_loss(ptr(pred), ptr(target), POS_WEIGHT, 1 if pred_is_prob else 0, ptr(loss), ptr(dlog), ptr(counts), ptr(loss_workspace(pred.device)),
                      pred.shape[0] * pred.shape[1])
    return loss, dlog


class _WeightedBCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, counts):
        loss, dlog = _loss_launch(pred, target, False, ctx.needs_input_grad[0], counts)
        ctx.dlog = dlog
        return loss

    @staticmethod
    def backward(ctx, gout):
        return ctx.dlog * gout, None, None


class WeightedLoss(nn.Module):
    """``nn.BCEWithLogitsLoss(pos_weight=(10, 10))`` with mean reduction (train_layout.py:94-97) as one launch that also produces the
    gradient and, when ``counts`` (int64 [6], device) is given, the counts ``LayoutAccuracyStats.update_counts`` consumes."""

    def forward(self, pred: torch.Tensor, target: torch.Tensor, counts: torch.Tensor | None = None) -> torch.Tensor:
        return _WeightedBCE.apply(pred, target, counts)


def weighted_loss() -> WeightedLoss:
    return WeightedLoss()


class LayoutAccuracyStats:
    """Running precision / recall of the line-start and line-end classes (train_layout.py:38-91).  The sums live on the device (fp64 sums of
    the reference's fp32 ratios) and are read by ``summary()``, ``stats_dict()`` and the ``*_precision_recall()`` methods only."""

    def __init__(self):
        self.updates = 0
        self._sums = None    # device fp64 [5]: the four running sums | number of updates
        self._counts = None  # device int64 [6], scratch of update()

    def _state(self, dev):
        if self._sums is None:
            self._sums = torch.zeros(5, dtype=torch.float64, device=dev)
            self._counts = torch.zeros(6, dtype=torch.int64, device=dev)
        return self._sums, self._counts

    def update(self, pred: torch.Tensor, target: torch.Tensor):
        """``pred``: probabilities (N, W, 2), thresholded at 0.5 as the reference does.  Two launches, no device-to-host copy."""
        sums, counts = self._state(pred.device)
        _loss_launch(pred, target, True, False, counts)
        self.update_counts(counts)

    def update_counts(self, counts: torch.Tensor):
        """Add one batch given the loss launch's counts (int64 [6]: per class true / predicted / target positives).  No device-to-host copy."""
        sums, _ = self._state(counts.device)
        self.updates += 1
        lib().layout_stats_update(ptr(counts), ptr(sums))

    def _means(self):
        if self._sums is None:
            raise ZeroDivisionError("no updates")
        s = self._sums.tolist()  # the one host synchronisation
        return [v / self.updates for v in s[:4]]

    def line_start_precision_recall(self) -> tuple[float, float]:
        m = self._means()
        return (m[0], m[1])

    def line_end_precision_recall(self) -> tuple[float, float]:
        m = self._means()
        return (m[2], m[3])

    def summary(self) -> str:
        m = self._means()
        return f"line start prec/recall {m[0]:.3f}/{m[1]:.3f} line end prec/recall {m[2]:.3f}/{m[3]:.3f}"

    def stats_dict(self) -> dict:
        m = self._means()
        return {"line_start_precision": m[0], "line_start_recall": m[1], "line_end_precision": m[2], "line_end_recall": m[3]}


def make_optimizer(model: LayoutModel) -> Adam:
    return Adam(model.parameters(), lr=3e-4)  # train_layout.py:223


def train_step(model, optimizer, batch, device, loss_fn: WeightedLoss | None = None, stats: LayoutAccuracyStats | None = None) -> torch.Tensor:
    """One iteration of train_layout.py:122-136.  ``batch`` = (input (N, W, 4), target (N, W, 2)).  Returns the device loss."""
    inp, target = [x.to(device, non_blocking=True) for x in batch]
    loss_fn = loss_fn or weighted_loss()
    optimizer.zero_grad()
    pred = model(inp)
    counts = stats._state(pred.device)[1] if stats is not None else None
    loss = loss_fn(pred, target, counts)
    loss.backward()
    if stats is not None:
        stats.update_counts(counts)  # (clamp(sigmoid(pred), 0, 1) >= 0.5, thresholded inside the loss launch)
    optimizer.step()
    return loss.detach()


def train(epoch: int, device, dataloader, model, optimizer) -> tuple[float, LayoutAccuracyStats]:
    """One epoch of training with the reference's signature (train_layout.py:100-139): (mean loss, statistics)."""
    model.train()
    loss_fn = weighted_loss()
    stats = LayoutAccuracyStats()
    total = torch.zeros((), dtype=torch.float64, device=device)
    n = 0
    for batch in dataloader:
        total += train_step(model, optimizer, batch, device, loss_fn, stats)
        n += 1
    return float(total.item()) / n, stats


def test(device, dataloader, model) -> tuple[float, LayoutAccuracyStats]:
    """Validation with the reference's signature (train_layout.py:142-171).  Like the reference it applies the sigmoid to the model output and
    feeds those PROBABILITIES to the logits loss (train_layout.py:164-166): that is the number the reference reports, kept as it is."""
    model.eval()
    stats = LayoutAccuracyStats()
    total = torch.zeros((), dtype=torch.float64, device=device)
    n = 0
    with torch.no_grad():
        for batch in dataloader:
            inp, target = [x.to(device, non_blocking=True) for x in batch]
            pred = model(inp).sigmoid()
            counts = stats._state(pred.device)[1]
            loss, _ = _loss_launch(pred, target, True, False, counts)
            stats.update_counts(counts)
            total += loss
            n += 1
    return float(total.item()) / n, stats


N_WORDS = 500    # train_layout.py:203-205: words used from each page; inputs and targets are padded to this length
BATCH_SIZE = 64  # train_layout.py:218
CHECKPOINT_FILE = "text-layout-checkpoint.pt"


def main(argv=None):
    """The reference's training script (train_layout.py:186-319) without wandb: same arguments, constants, print lines and checkpoint file."""
    parser = ArgumentParser(description="Train text layout model.")
    parser.add_argument("data_dir")
    parser.add_argument("--checkpoint", type=str, help="Model checkpoint to load")
    parser.add_argument("--export", type=str, help="Export model to ONNX format")
    parser.add_argument("--max-epochs", type=int, help="Maximum number of epochs to train for")
    parser.add_argument("--validate-only", action="store_true", help="Run validation only")
    args = parser.parse_args(argv)

    if not torch.cuda.is_available():
        raise RuntimeError("ocrs_models_amd.train_layout runs on MI355X only (no CPU path)")
    torch.manual_seed(1234)
    normalize_coords = False
    max_jitter = 10  # max random translation of the training pages

    device = torch.device("cuda")
    model = LayoutModel(return_probs=False, pos_embedding="sin").to(device)
    optimizer = make_optimizer(model)
    scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lr_scale_for_epoch)
    train_dataset = WebLayout(args.data_dir, max_jitter=max_jitter, normalize_coords=normalize_coords, randomize=True, padded_size=N_WORDS,
                              train=True, device=device)
    train_dataloader = DeviceWebLayoutLoader(train_dataset, batch_size=BATCH_SIZE, shuffle=True)
    val_dataset = WebLayout(args.data_dir, normalize_coords=normalize_coords, randomize=False, padded_size=N_WORDS, train=False, device=device)
    val_dataloader = DeviceWebLayoutLoader(val_dataset, batch_size=BATCH_SIZE, shuffle=True)

    total_params = sum(p.numel() for p in model.parameters() if p.requires_grad)
    print(f"Model param count {total_params}")

    epoch = 0
    if args.checkpoint:
        checkpoint = load_checkpoint(args.checkpoint, model, optimizer, device)
        epoch = checkpoint["epoch"]

    if args.export:
        from .export import export_onnx

        dummy_input, dummy_target = next(iter(train_dataloader))
        export_onnx(model, args.export, dummy_input[0:1])
        return

    if args.validate_only:
        val_loss, val_stats = test(device, val_dataloader, model)
        print(f"Epoch {epoch} val stats: {val_stats.summary()}")
        return

    best_val_loss = float("inf")
    while args.max_epochs is None or epoch < args.max_epochs:
        train_loss, train_stats = train(epoch, device, train_dataloader, model, optimizer)
        val_loss, val_stats = test(device, val_dataloader, model)
        lr = optimizer.state_dict()["param_groups"][0]["lr"]

        print(f"Epoch {epoch} train loss {train_loss} val loss {val_loss}")
        print(f"Epoch {epoch} train stats: {train_stats.summary()}")
        print(f"Epoch {epoch} val stats: {val_stats.summary()}")
        print(f"Epoch {epoch} lr {lr}")

        if val_loss < best_val_loss:
            best_val_loss = val_loss
            save_checkpoint(CHECKPOINT_FILE, model, optimizer, epoch=epoch)

        scheduler.step()
        epoch += 1


if __name__ == "__main__":
    main()
