"""flair_amd — MI355X-native segmentation hot path of FLAIR-1 (U-Net/ResNet34 fwd+bwd, CE/argmax/IoU head).

Host code is Python on PyTorch-ROCm (device memory, streams, torch.distributed); every FLOP of the path
runs in hand-written HIP kernels inside ``libflair_hip.so`` (C ABI: include/flair_hip.h).
"""
from . import _lib
from .unet import Unet, create_model
from .model import FLAIR_ModelFactory, MetadataMLP
from .segformer import SegformerForSemanticSegmentation
from .upernet import UperNetForSemanticSegmentation
from .head import FusedCrossEntropyLoss, FusedSegLoss, MulticlassJaccardIndex, MeanMetric
from .losses import SegLoss
from .task_module import segmentation_task_training, segmentation_task_predict
from .train import SegTrainer, bucket_ranges, allreduce_buckets, shard_indices, reduce_validation_state
from .data_feed import TileFeed, draw_d4
from .tta import tta_codes, tta_predict
from . import optim
from . import losses
from . import checkpoint, metrics, raster_reader, raster_writer, tasks_utils, tile_loader, tta, writer, zone_detect, zone_metrics
from .tile_loader import TileLoader, read_tiles
from .raster_writer import read_geo_tags, tiled_tiff_header, tiled_tiff_ifd, write_raster
from .raster_reader import RasterDecodeError, RasterLayout, UnsupportedRaster, raster_layout, read_raster

__all__ = ["Unet", "create_model", "FLAIR_ModelFactory", "MetadataMLP", "FusedCrossEntropyLoss", "SegformerForSemanticSegmentation",
           "UperNetForSemanticSegmentation",
           "MulticlassJaccardIndex", "MeanMetric", "segmentation_task_training", "segmentation_task_predict",
           "SegTrainer", "bucket_ranges", "allreduce_buckets", "shard_indices", "reduce_validation_state", "TileFeed", "draw_d4", "checkpoint", "metrics", "tasks_utils",
           "writer", "zone_detect", "zone_metrics", "raster_writer", "write_raster", "read_geo_tags", "tiled_tiff_ifd", "tiled_tiff_header",
           "raster_reader", "read_raster", "raster_layout", "RasterLayout", "UnsupportedRaster", "RasterDecodeError",
           "tile_loader", "TileLoader", "read_tiles", "tta", "tta_codes", "tta_predict", "optim", "losses", "SegLoss", "FusedSegLoss"]
