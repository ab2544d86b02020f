"""Detection training step, the body of the reference's ``train()`` loop (ocrs_models/train_detection.py:82-111):
H2D copy, forward, balanced BCE, zero_grad, backward, Adam step -- without the per-step ``loss.item()`` host syncs
(the loss stays a device scalar; callers read it when they need it) -- and the validation loop ``test()``
(ocrs_models/train_detection.py:144-195): eval-mode forward (running-statistics BatchNorm) + the same loss.  ``main`` is the reference's
training script (train_detection.py:293-489) on the device-resident datasets of ocrs_models_amd/datasets/."""
from __future__ import annotations

import os
import shutil
from argparse import ArgumentParser, BooleanOptionalAction

import torch

from .checkpoint import load_checkpoint, save_checkpoint  # noqa: F401  (train_detection.py:198-215)
from .losses import balanced_cross_entropy_loss, fused_head_backward
from .models import DetectionModel
from .optim import Adam


def make_optimizer(model: DetectionModel) -> Adam:
    return Adam(model.parameters())  # train_detection.py:378


def train_step(model, optimizer, batch: dict, device, loss_fn=balanced_cross_entropy_loss) -> torch.Tensor:
    """One iteration of train_detection.py:82-98.  ``batch`` = {"image": (B,1,H,W), "text_mask": (B,1,H,W), ...}."""
    img = batch["image"].to(device, non_blocking=True)
    masks = batch["text_mask"].to(device, non_blocking=True)
    pred_masks = model(img)
    loss = loss_fn(pred_masks, masks)
    optimizer.zero_grad()
    if loss_fn is balanced_cross_entropy_loss:
        # pred's only consumer is the built-in loss: its backward is folded into the network's head backward (losses.fused_head_backward)
        with fused_head_backward():
            loss.backward()
    else:
        loss.backward()
    optimizer.step()
    return loss.detach()


def train(epoch: int, device, dataloader, model, loss_fn, optimizer) -> float:
    """Epoch loop with the reference's signature (train_detection.py:66-116); one host sync per epoch."""
    model.train()
    total = torch.zeros((), device=device)
    n = 0
    for batch in dataloader:
        total += train_step(model, optimizer, batch, device, loss_fn)
        n += 1
    return float(total.item()) / max(n, 1)


def binarize_mask(mask: torch.Tensor, threshold: float = 0.5) -> torch.Tensor:
    """train_detection.py:33-34."""
    return torch.where(mask > threshold, 1.0, 0.0)


def mean(values: list[float]) -> float:
    return sum(values) / len(values)


def get_metric_means(metrics_dicts: list[dict[str, float]]) -> dict[str, float]:
    """Means of all metrics in a list of dicts; a key missing from a dict counts as 0 (train_detection.py:122-137)."""
    if not len(metrics_dicts):
        return {}
    keys = set(k for md in metrics_dicts for k in md.keys())
    return {k: mean([md.get(k, 0.0) for md in metrics_dicts]) for k in keys}


def test(device, dataloader, model, loss_fn=balanced_cross_entropy_loss, metrics_fn="default") -> tuple[float, dict[str, float]]:
    """Validation loop with the reference's return value: (mean pixel-level loss, mean word-level metrics).

    The forward and the loss run on the GPU in eval mode under ``torch.inference_mode()``; the loss is accumulated on the device (one
    host sync per epoch).  The word-level metrics (precision / recall / merged_frac / split_frac per image, averaged) are computed on
    the CPU per image exactly where the reference does (train_detection.py:177-184) by ``postprocess.mask_metrics`` -- a numpy
    restatement of the reference's cv2 + shapely post-processing (postprocess.py:11-36, 102-187; neither library is installed here, so
    its parity is unpinned: see ocrs_models_amd/postprocess.py).  ``metrics_fn(bin_pred_mask_cpu, bin_target_mask_cpu) -> dict`` replaces
    it (e.g. the reference's own functions); ``metrics_fn=None`` skips the metrics (empty dict).  ``metrics_fn="device"`` computes the same
    four metrics on the GPU (``postprocess.batch_mask_metrics`` on the device-resident prediction and target, running sums on the device):
    no per-batch host copy, and the loop's one host sync returns the same dict as the default path.
    """
    device_metrics = isinstance(metrics_fn, str) and metrics_fn == "device"
    if isinstance(metrics_fn, str) and metrics_fn == "default":
        from .postprocess import mask_metrics as metrics_fn
    elif device_metrics:
        from .postprocess import METRIC_KEYS, batch_mask_metrics
    model.eval()
    n_batches = 0
    n_images = 0
    metrics = []
    with torch.inference_mode():
        total = torch.zeros((), device=device)
        msum = torch.zeros(4, dtype=torch.float64, device=device) if device_metrics else None
        for batch in dataloader:
            img = batch["image"].to(device, non_blocking=True)
            masks = batch["text_mask"].to(device, non_blocking=True)
            pred_masks = model(img)
            total += loss_fn(pred_masks, masks)
            n_batches += 1
            if device_metrics:
                msum += batch_mask_metrics(pred_masks, masks).sum(0)
                n_images += pred_masks.shape[0]
            elif metrics_fn is not None:
                bin_pred_masks = binarize_mask(pred_masks).cpu()
                bin_masks = binarize_mask(masks).cpu()
                for item_index, bin_pred_mask in enumerate(bin_pred_masks):
                    metrics.append(metrics_fn(bin_pred_mask, bin_masks[item_index]))
    if device_metrics:
        vals = torch.cat([total.double().reshape(1), msum]).tolist()  # the one host sync of the loop
        return vals[0] / max(n_batches, 1), ({k: v / n_images for k, v in zip(METRIC_KEYS, vals[1:])} if n_images else {})
    return float(total.item()) / max(n_batches, 1), get_metric_means(metrics)


def format_metrics(metrics: dict[str, float]) -> dict[str, str]:
    """train_detection.py:140-141."""
    return {k: f"{v:.3f}" for k, v in metrics.items()}


def save_img_and_predicted_mask(basename: str, img_filename: str, img: torch.Tensor, pred_masks, target_masks=None):
    """train_detection.py:37-60 with PIL in place of torchvision's to_pil_image (a float (1, H, W) tensor: mul(255) then the byte cast)."""
    from PIL import Image

    def to_pil(t):
        return Image.fromarray(t.detach().float().mul(255).byte().cpu().numpy().reshape(t.shape[-2:]), "L")

    shutil.copyfile(img_filename, f"{basename}_input.png")
    to_pil(img + 0.5).save(f"{basename}_input_scaled.png")
    for i, pred_mask in enumerate(pred_masks):
        to_pil(pred_mask).save(f"{basename}_pred_mask_{i}.png")
    if target_masks is not None:
        for i, target_mask in enumerate(target_masks):
            to_pil(target_mask).save(f"{basename}_mask_{i}.png")


class _DebugImages:
    """A loader that keeps the reference's debug images of every batch it hands out (train_detection.py:102-109, 186-189): written once
    the consumer comes back for the next batch, from an eval-mode forward of the first image (the training forward's own prediction stays
    inside ``train_step``; a second training-mode forward would move the BatchNorm statistics)."""

    def __init__(self, loader, model, basename: str):
        self.loader, self.model, self.basename = loader, model, basename

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            yield batch
            was_training = self.model.training
            self.model.eval()
            with torch.no_grad():
                pred = self.model(batch["image"][:1])
            self.model.train(was_training)
            save_img_and_predicted_mask(self.basename, batch["path"][0], batch["image"][0], pred[0], [batch["text_mask"][0]])


CHECKPOINT_FILE = "text-detection-checkpoint.pt"


def prepare_loaders(dataset_type: str, data_dir: str, batch_size: int, max_images=None, augment=True, device="cuda", mask_size=None):
    """The two datasets and loaders of train_detection.py:326-366: the training loader shuffles, the validation loader does not; both
    datasets get ``prepare_transform(mask_size, augment)`` as the reference gives its one transform to both."""
    from .datasets import DDI100, DevicePageLoader, HierText

    if dataset_type == "ddi":
        load_dataset = DDI100
    elif dataset_type == "hiertext":
        load_dataset = HierText
    else:
        raise Exception(f"Unknown dataset type {dataset_type}")
    validation_max_images = max(10, int(max_images * 0.1)) if max_images else None
    train_dataset = load_dataset(data_dir, augment=augment, train=True, max_images=max_images, device=device, mask_size=mask_size)
    train_dataloader = DevicePageLoader(train_dataset, batch_size=batch_size, shuffle=True)
    val_dataset = load_dataset(data_dir, augment=augment, train=False, max_images=validation_max_images, device=device, mask_size=mask_size)
    val_dataloader = DevicePageLoader(val_dataset, batch_size=batch_size)
    return train_dataset, train_dataloader, val_dataset, val_dataloader


def main(argv=None):
    """The reference's training script (train_detection.py:293-489) without wandb: same arguments, seed, validation-size rule, print lines
    and checkpoint file.  Validation keeps its word-level metrics on the GPU (``test(..., metrics_fn="device")``)."""
    parser = ArgumentParser(description="Train text detection model.")
    parser.add_argument("dataset_type", type=str, choices=["ddi", "hiertext"], help="Format of dataset")
    parser.add_argument("data_dir")
    parser.add_argument("--batch-size", type=int, default=4, help="Batch size")
    parser.add_argument("--checkpoint", type=str, help="Model checkpoint to load")
    parser.add_argument("--debug-images", action="store_true", help="Save debugging images during training")
    parser.add_argument("--export", type=str, help="Export model to ONNX format")
    parser.add_argument("--max-epochs", type=int, help="Maximum number of epochs to train for")
    parser.add_argument("--max-images", type=int, help="Maximum number of images to load")
    parser.add_argument("--validate-only", action="store_true", help="Run validation on an existing model")
    parser.add_argument("--augment", default=True, action=BooleanOptionalAction, help="Enable data augmentation")
    args = parser.parse_args(argv)

    if not torch.cuda.is_available():
        raise RuntimeError("ocrs_models_amd.train_detection runs on MI355X only (no CPU path)")
    torch.manual_seed(1234)
    device = torch.device("cuda", torch.cuda.current_device())

    train_dataset, train_dataloader, val_dataset, val_dataloader = prepare_loaders(args.dataset_type, args.data_dir, args.batch_size,
                                                                                   args.max_images, args.augment, device)
    print(f"Training dataset: images {len(train_dataset)} in {len(train_dataloader)} batches")
    print(f"Validation dataset: images {len(val_dataset)} in {len(val_dataloader)} batches")

    model = DetectionModel().to(device)
    optimizer = make_optimizer(model)
    total_params = sum(p.numel() for p in model.parameters() if p.requires_grad)
    print(f"Model param count: {total_params}")

    epochs_without_improvement = 0
    min_train_loss = 1.0
    epoch = 0
    if args.checkpoint:
        checkpoint = load_checkpoint(args.checkpoint, model, optimizer, device)
        epoch = checkpoint["epoch"]

    if args.export:
        if not args.checkpoint:
            raise Exception("ONNX export requires a checkpoint to load")
        import importlib.util

        if importlib.util.find_spec("onnx") is None:
            parser.exit(1, "--export needs the onnx package, which is not installed\n")
        from .export import export_onnx

        test_batch = next(iter(val_dataloader))
        export_onnx(model, args.export, test_batch["image"][0:1].to(device))
        return

    train_loader, val_loader = train_dataloader, val_dataloader
    if args.debug_images:
        train_loader = _DebugImages(train_dataloader, model, "train-sample")
        val_loader = _DebugImages(val_dataloader, model, "test-sample")

    if args.validate_only:
        if not args.checkpoint:
            parser.exit(1, "Existing model should be specified with --checkpoint when using --validate-only")
        val_loss, val_metrics = test(device, val_loader, model, balanced_cross_entropy_loss, metrics_fn="device")
        print(f"Validation loss {val_loss:.4f}")
        print("Validation metrics:", format_metrics(val_metrics))
        return

    while args.max_epochs is None or epoch < args.max_epochs:
        train_loss = train(epoch, device, train_loader, model, balanced_cross_entropy_loss, optimizer)
        val_loss, val_metrics = test(device, val_loader, model, balanced_cross_entropy_loss, metrics_fn="device")
        print(f"Epoch {epoch} train loss {train_loss:.4f} validation loss {val_loss:.4f}")
        print(f"Epoch {epoch} validation metrics:", format_metrics(val_metrics))
        if train_loss < min_train_loss:
            min_train_loss = train_loss
            epochs_without_improvement = 0
            save_checkpoint(CHECKPOINT_FILE, model, optimizer, epoch=epoch)
        else:
            epochs_without_improvement += 1
        if epochs_without_improvement > 3:
            print(f"Stopping after {epochs_without_improvement} epochs without train loss improvement")
        epoch += 1


if __name__ == "__main__":
    main()
