"""ocrs_models_amd -- MI355X-native (gfx950) detection / recognition / layout train-step hot path of
robertknight/ocrs-models: same nn.Module and loss signatures as ocrs_models/models.py,
train_detection.py, train_rec.py and train_layout.py, executed by hand-written HIP kernels (libocrs_hip.so)."""
from . import checkpoint, export, graph, input_pipeline, optim, sampler, text  # noqa: F401
from .losses import CTCLoss, balanced_cross_entropy_loss  # noqa: F401
from .models import DetectionModel  # noqa: F401
from .recognition import RecognitionModel  # noqa: F401
from .layout import LayoutModel  # noqa: F401
from . import losses, train_detection, train_layout, train_rec  # noqa: F401,E402
from . import inference  # noqa: F401,E402
from .inference import (MASK_SIZE, SHRINK_DISTANCE, ReadingOrder, TextLines, binarize_resize, binarize_resize_pages, cc_quads_pages, crop_plan, crops_to_batches,  # noqa: F401,E402
                        detect_words, detect_words_batch, expand_quads, find_lines, find_lines_pages, gather_page_quads, ocr_lines, ocr_page,
                        ocr_pages, pack_pages, page_text, read_lines, read_words, reading_order, recognize_crops, rectify_crops, rectify_crops_pages, split_by_page)
from .inference import TilePlan, TileTables, binarize_resize_tiles, tile_batch, tile_plan, tile_tables  # noqa: F401,E402
