"""The device-resident datasets, one module per family, named as the reference names them (ocrs_models/datasets/): ``web_layout`` (the layout
model's WebLayout), ``hiertext`` (HierTextRecognition's text lines, HierText's pages, the evaluation's ground truth), ``ddi100``; ``pages``
holds the page store that HierText and DDI100 share, ``util`` what all of them share."""
from .ddi100 import DDI100, DDI100Unpickler  # noqa: F401
from .hiertext import (MAX_LINE_VERTICES, DeviceLineLoader, HierText, HierTextRecognition, WordTruth, from_words,  # noqa: F401
                       generate_json_lines_annotations, generate_text_line_annotations, hiertext_line_truth, hiertext_text_lines,
                       hiertext_word_polygons, hiertext_word_truth)
from .pages import BAND_ROWS, DevicePageLoader  # noqa: F401
from .util import (MAX_POLYGON_VERTICES, SHRINK_DISTANCE, IndexLoader, bounding_box_size, decode_pages, line_bounding_box,  # noqa: F401
                   read_gray)
from .web_layout import DeviceWebLayoutLoader, WebLayout, parse_page, select_files  # noqa: F401
