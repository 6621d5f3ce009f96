"""Feature extraction on the device: Database::ExtractImageFeatures (SfM/src/database.cc:289-349) with the VLFeat extractor,
VLSiftExtractor::Run without its optional resize (SfM/src/feature/feature_extractor_vl_sift.cpp:75-216), through
msfm_scalespace_create + msfm_descset_extract (include/msfm.h states the definitions; parity with VLFeat is unpinned).

No keypoint and no descriptor is made on the host: the frames alone pass through it between the detection and the descriptor
kernel.  The rows lie in the descriptor set as `DescSet.words`, `pairsel.select_pairs_from_descriptors` and
`DescSet.match_pairs` read them."""
import numpy as np

from . import capi, featurefiles


def extract_image_features(ds: capi.DescSet, image, gray, n_octaves=4, n_levels=5, peak_thresh=0.0, edge_thresh=10.0, max_frames=65535,
                           quantize=False, fold=None, info=None):
    """The features of one uint8 image [h][w] into image `image` of the set `ds`: scale space, detection, descriptors; the
    scale space is released again.  -> the stats dict of `DescSet.extract`.  With fold, `<fold>/<image>_feature` is written as the
    reference writes it (featurefiles.write_image_feature; info: its dict, rows and cols default to the image's)."""
    gray = np.asarray(gray)
    with ds.ctx.scalespace(gray, n_octaves, n_levels) as ss:
        stats = ds.extract(image, ss, peak_thresh, edge_thresh, max_frames, quantize)
    if fold is not None:
        rows, xy = ds.fetch(image)
        meta = dict(rows=gray.shape[0], cols=gray.shape[1])
        meta.update(info or {})
        featurefiles.write_image_feature(fold, image, meta, xy if xy is not None else np.zeros((0, 2), np.float32), rows)
    return stats


def extract_all(ctx: capi.Context, grays, fold=None, infos=None, **options):
    """extract_image_features for every image of `grays` into a new descriptor set.  -> the `DescSet`; its `extract_stats` is the list of the
    images' stats dicts.  options: the further arguments of extract_image_features."""
    ds = ctx.descset([np.zeros((0, 128), np.float32)] * len(grays))
    try:
        ds.extract_stats = [extract_image_features(ds, i, g, fold=fold, info=None if infos is None else infos[i], **options) for i, g in enumerate(grays)]
    except Exception:
        ds.close()
        raise
    return ds
