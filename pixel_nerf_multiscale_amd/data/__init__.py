"""
The data layer: upstream pixelNeRF's data package (src/data: get_split_dataset, SRNDataset, DVRDataset) restated for this
package's drivers, plus ResidentSplit, which keeps a whole split on the card as the bytes its image files hold.

PARITY UNPINNED.  The reference fork's scripts import src/data and do not ship it, and upstream's code is not available where
this package is developed, so nothing here was compared against either: the specification is the on-disk layouts the class
docstrings state (SRN cars / chairs, the ShapeNet sub-format of DVR / NMR, and the DTU sub-format of DVR).  Where evalio.metrics_map already relies on a
layout fact ("image" / "rgb" folders, "<list_name>.lst"), this package agrees with it.

Items come in two modes.  as_bytes=False (the default) is what evaluate, evaluate_approx, gen_video and vis_step take:
float32 images (NV, 3, H, W).  as_bytes=True is for train.calc_losses: uint8 images (NV, H, W, 3), a quarter of the bytes,
converted on the device only where a step needs them (util.train_batch_u8, util.views_to_tensor_u8) to the bits the float
item holds.

Another image_size.  The dataset classes read what the files hold and refuse a foreign image_size; the resampling
(upstream's F.interpolate(mode="area")) is done on the device instead: ResidentSplit(image_size=...) builds its pool at the
new size, and ResizedDataset wraps any dataset so that its items come at that size (util.resize_area_u8, util.resize_area,
util.resize_bbox, util.resize_intrinsics).
"""
from . import synthetic
from .dtu import ColorJitter, DTUDataset
from .dvr import DVRDataset
from .resident import ResidentSplit
from .resized import ResizedDataset
from .srn import SRNDataset
from .synthetic import SyntheticShapes

__all__ = ["get_split_dataset", "SRNDataset", "DVRDataset", "DTUDataset", "ColorJitter", "ResidentSplit", "ResizedDataset",
           "SyntheticShapes"]


def get_split_dataset(dataset_type, datadir, want_split="all", training=True, **kwargs):
    """The dataset(s) of one folder.  dataset_type "srn" -> SRNDataset, "dvr" -> DVRDataset, "dvr_gen" -> DVRDataset with the
    "gen_" object lists, "dtu" -> DTUDataset, "synthetic" -> SyntheticShapes (no folder: datadir is ignored, n_objects is
    required, and val / test default to max(1, n_objects // 8) objects; see synthetic.split); want_split "train" | "val" | "test" returns that one set, anything else the
    (train, val, test) triple.  kwargs go to the dataset class (image_size, world_scale, balanced, as_bytes, ...).  `training`
    is upstream's switch: for "dtu" it sets max_imgs=49 (a training item is a random 49 of a scan's views); the other types
    ignore it.  "dvr_dtu", upstream's name for the DTU sub-format, stays refused, because upstream reads it through cv2 and
    nothing here was compared against that: "dtu" is the working name of this package's own reading of the layout."""
    if dataset_type == "synthetic":
        return synthetic.split(want_split, **kwargs)
    if dataset_type == "srn":
        cls, flags = SRNDataset, {}
    elif dataset_type == "dvr":
        cls, flags = DVRDataset, {}
    elif dataset_type == "dvr_gen":
        cls, flags = DVRDataset, {"list_prefix": "gen_"}
    elif dataset_type == "dtu":
        cls, flags = DTUDataset, ({"max_imgs": 49} if training else {})
    elif dataset_type == "dvr_dtu":
        raise NotImplementedError("dataset type 'dvr_dtu': the DTU sub-format decomposes its projection matrices with "
                                  "cv2.decomposeProjectionMatrix, and this package does not depend on cv2")
    elif dataset_type == "multi_obj":
        raise NotImplementedError("dataset type 'multi_obj': the multi-object layout (transforms.json per scene) is not "
                                  "specified by anything in this package and no driver here uses it")
    else:
        raise NotImplementedError(f"unsupported dataset type {dataset_type!r}")
    flags.update(kwargs)
    if want_split in ("train", "val", "test"):
        return cls(datadir, stage=want_split, **flags)
    return tuple(cls(datadir, stage=stage, **flags) for stage in ("train", "val", "test"))
