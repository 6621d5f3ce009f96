"""The reference's per-image feature file and its Bundler export, so that datasets produced by
the reference's extraction stage can feed libmsfm and libmsfm's results can feed the reference's downstream tools.

  <output_fold>/<idx>_feature   binary (Database::WriteoutImageFeature / ReadinImageFeatures, SfM/src/database.cc:490-541, :352-423):
      int32 rows, int32 cols, float32 zoom_ratio, float32 f_mm, float32 f_pixel, float32 gps_latitude, float32 gps_longitude,
      int32 len + bytes cam_maker, int32 len + bytes cam_model,
      int32 n, float32[2n] keypoints CENTRED (x - cols/2.0, y - rows/2.0; the writer centres, the reader does not undo it),
      int32 rows, int32 cols, int32 OpenCV type, raw descriptor bytes (CV_32FC1 = 5 for SIFT, database.cc:412-418)
  bundle.rd.out                 text, "# Bundle file v0.3" (IncrementalSfM::SaveForCMVS, sfm_incremental.cc:1302-1353): fixed, 8 decimals;
      per camera f k1 k2 / R (row-major, 9 values) / t; per point X Y Z / 255 255 255 / view list, where the reference
      truncates the image coordinates to int before printing them as float (:1342-1345).
  <output_fold>/<idx>_words     binary (Database::WriteoutWordsForImage / ReadinWordsForImage, database.cc:869-945): int32 count, int32[count]
      word ids and float32[count] weights of the image's bag of words, int32 max_words_id_, int32 num_pts, int32[num_pts] the word
      id of every feature.  An image without words is an EMPTY file (:911).
  <output_fold>/voctree         binary (Database::WriteoutVocabularyTree / ReadinVocabularyTree, database.cc:679-735): fbow's params and its
      block memory; the layout is spelled out above read_voctree / write_voctree below.
  sfm_openmvs.txt, temp_result  text: the OpenMVS hand-over (:1147-1245) and the reconstruction checkpoint (:1465-1749), below.
Native little-endian, as the reference writes them with ofstream::write."""
import os
import struct

import numpy as np

CV_8U, CV_32F = 0, 5
_ELEM = {0: (np.uint8, 1), 1: (np.int8, 1), 2: (np.uint16, 2), 3: (np.int16, 2), 4: (np.int32, 4), 5: (np.float32, 4), 6: (np.float64, 8)}


def feature_file(fold, idx):
    return os.path.join(fold, "%d_feature" % idx)


def write_image_feature(fold, idx, info, keypoints_px, descriptors):
    """info: dict(rows, cols, zoom_ratio, f_mm, f_pixel, gps_latitude, gps_longitude, cam_maker, cam_model);
    keypoints_px [n][2] in image pixels (centred on write, database.cc:522-527); descriptors [n][d] float32 or uint8."""
    kp = np.asarray(keypoints_px, dtype=np.float64).reshape(-1, 2)
    d = np.ascontiguousarray(descriptors)
    if d.dtype not in (np.float32, np.uint8):
        d = d.astype(np.float32)
    cv_type = CV_32F if d.dtype == np.float32 else CV_8U
    centred = np.empty((len(kp), 2), dtype=np.float32)
    centred[:, 0] = kp[:, 0] - info["cols"] / 2.0
    centred[:, 1] = kp[:, 1] - info["rows"] / 2.0
    maker, model = info.get("cam_maker", "").encode(), info.get("cam_model", "").encode()
    with open(feature_file(fold, idx), "wb") as f:
        f.write(struct.pack("<ii5f", int(info["rows"]), int(info["cols"]), info.get("zoom_ratio", 1.0), info.get("f_mm", 0.0),
                            info.get("f_pixel", 0.0), info.get("gps_latitude", 0.0), info.get("gps_longitude", 0.0)))
        f.write(struct.pack("<i", len(maker)) + maker)
        f.write(struct.pack("<i", len(model)) + model)
        f.write(struct.pack("<i", len(centred)))
        centred.tofile(f)
        f.write(struct.pack("<iii", d.shape[0], d.shape[1] if d.ndim > 1 else 1, cv_type))
        d.tofile(f)


def read_image_feature(fold, idx):
    """-> info dict, keypoints [n][2] float32 (centred pixels, as stored), descriptors [rows][cols]."""
    with open(feature_file(fold, idx), "rb") as f:
        rows, cols, zoom, f_mm, f_px, lat, lon = struct.unpack("<ii5f", f.read(28))
        n = struct.unpack("<i", f.read(4))[0]
        maker = f.read(n).decode()
        n = struct.unpack("<i", f.read(4))[0]
        model = f.read(n).decode()
        npts = struct.unpack("<i", f.read(4))[0]
        kp = np.fromfile(f, dtype=np.float32, count=2 * npts).reshape(-1, 2)
        drows, dcols, cv_type = struct.unpack("<iii", f.read(12))
        depth, channels = cv_type & 7, (cv_type >> 3) + 1
        dt, _ = _ELEM[depth]
        desc = np.fromfile(f, dtype=dt, count=drows * dcols * channels).reshape(drows, dcols * channels)
    info = dict(rows=rows, cols=cols, zoom_ratio=zoom, f_mm=f_mm, f_pixel=f_px, gps_latitude=lat, gps_longitude=lon, cam_maker=maker,
                cam_model=model)
    return info, kp, desc


def words_file(fold, idx):
    return os.path.join(fold, "%d_words" % idx)


def write_words(fold, idx, bow_ids, bow_weights, max_words_id, word_id):
    """bow_ids / bow_weights: the image's fbow vector (ascending id, as std::map iterates); word_id: the word of every feature.
    bow_ids None: an image without words, an empty file."""
    with open(words_file(fold, idx), "wb") as f:
        if bow_ids is None:
            return
        ids, w = np.asarray(bow_ids, dtype=np.int32).reshape(-1), np.asarray(bow_weights, dtype=np.float32).reshape(-1)
        if len(ids) != len(w):
            raise ValueError("one weight per word")
        wid = np.asarray(word_id, dtype=np.int32).reshape(-1)
        f.write(struct.pack("<i", len(ids)))
        ids.tofile(f)
        w.tofile(f)
        f.write(struct.pack("<ii", int(max_words_id), len(wid)))
        wid.tofile(f)


def read_words(fold, idx):
    """-> (bow_ids, bow_weights, max_words_id, word_id), or (None, None, None, None) for an empty file."""
    with open(words_file(fold, idx), "rb") as f:
        head = f.read(4)
        if len(head) < 4:
            return None, None, None, None
        n = struct.unpack("<i", head)[0]
        ids = np.fromfile(f, dtype=np.int32, count=n)
        w = np.fromfile(f, dtype=np.float32, count=n)
        max_id, npts = struct.unpack("<ii", f.read(8))
        wid = np.fromfile(f, dtype=np.int32, count=npts)
    return ids, w, max_id, wid


def write_all_words(fold, fetched):
    """Every image's `<i>_words` from WordResult.fetch() (Database::BuildWords, database.cc:789-808): an image without words gets
    the empty file; the others record Database::max_words_id_ as it stands after them, the running maximum of image_max_id in
    image order from 0.  -> that running maximum per image [n]."""
    fo, bo = fetched["feat_off"], fetched["bow_off"]
    running, out = 0, []
    for i in range(len(fetched["has_words"])):
        if fetched["has_words"][i]:
            running = max(running, int(fetched["image_max_id"][i]))
            write_words(fold, i, fetched["bow_word"][bo[i]:bo[i + 1]], fetched["bow_weight"][bo[i]:bo[i + 1]], running,
                        fetched["word_id"][fo[i]:fo[i + 1]])
        else:
            write_words(fold, i, None, None, running, None)
        out.append(running)
    return np.array(out, dtype=np.int32)


# <output_fold>/voctree (Database::WriteoutVocabularyTree / ReadinVocabularyTree, database.cc:679-735): fbow's params without the
# descriptor name, then its block memory.
#   uint32 _aligment, uint32 _nblocks, uint64 _desc_size_bytes_wp, uint64 _block_size_bytes_wp, uint64 _feature_off_start,
#   uint64 _child_off_start, uint64 _total_size, int32 _desc_type, int32 _desc_size, uint32 _m_k, then _total_size bytes.
# Block b starts at b * _block_size_bytes_wp (fbow.h:155-193): uint16 N, uint16 isLeaf, uint32 parent block; descriptor i at
# _feature_off_start + i * _desc_size_bytes_wp; block_node_info i = (uint32 id_or_childblock, float32 weight) at
# _child_off_start + 8 i.  The offsets are read from the header, never assumed.
_VOC_HEAD = "<IIQQQQQiiI"
VOC_DIM = 128


def _round_up(x, a):
    return (x + a - 1) // a * a


def voctree_layout(k, alignment=32, feature_off_start=None, desc_size_bytes_wp=None):
    """A block layout for write_voctree: descriptors aligned to `alignment` behind the 8-byte block head, the node infos behind the
    k descriptors, the block padded to the alignment.  (fbow's own setParams is in its .cpp, which this project has not seen;
    any layout the header describes reads back the same.)"""
    wp = _round_up(4 * VOC_DIM, alignment) if desc_size_bytes_wp is None else int(desc_size_bytes_wp)
    fo = _round_up(8, alignment) if feature_off_start is None else int(feature_off_start)
    co = fo + k * wp
    return dict(alignment=alignment, desc_size_bytes_wp=wp, feature_off_start=fo, child_off_start=co,
                block_size_bytes_wp=_round_up(co + 8 * k, alignment))


def write_voctree(path, k, block_n, node_desc, node_link, node_weight, block_leaf=None, block_parent=None, layout=None):
    """block_n [nb]; node_desc [nb][k][128] float32; node_link [nb][k] uint32 (id_or_childblock); node_weight [nb][k] float32;
    block_leaf / block_parent [nb] (default 0); layout: voctree_layout(k, ...)."""
    bn = np.asarray(block_n, dtype=np.uint16).reshape(-1)
    nb, k = len(bn), int(k)
    nd = np.ascontiguousarray(node_desc, dtype=np.float32).reshape(nb, k, VOC_DIM)
    nl = np.asarray(node_link, dtype=np.uint32).reshape(nb, k)
    nw = np.asarray(node_weight, dtype=np.float32).reshape(nb, k)
    lay = voctree_layout(k) if layout is None else layout
    wp, fo, co, bs = lay["desc_size_bytes_wp"], lay["feature_off_start"], lay["child_off_start"], lay["block_size_bytes_wp"]
    if wp < 4 * VOC_DIM or fo < 8 or co < fo + k * wp or bs < co + 8 * k:
        raise ValueError("the layout's parts overlap")
    data = np.zeros((nb, bs), dtype=np.uint8)
    data[:, 0:2] = bn.view(np.uint8).reshape(nb, 2)
    data[:, 2:4] = np.zeros(nb, np.uint16).view(np.uint8).reshape(nb, 2) if block_leaf is None else \
        np.asarray(block_leaf, dtype=np.uint16).reshape(nb).view(np.uint8).reshape(nb, 2)
    data[:, 4:8] = np.zeros(nb, np.uint32).view(np.uint8).reshape(nb, 4) if block_parent is None else \
        np.asarray(block_parent, dtype=np.uint32).reshape(nb).view(np.uint8).reshape(nb, 4)
    for i in range(k):
        data[:, fo + i * wp: fo + i * wp + 4 * VOC_DIM] = np.ascontiguousarray(nd[:, i]).view(np.uint8).reshape(nb, 4 * VOC_DIM)
        data[:, co + 8 * i: co + 8 * i + 4] = np.ascontiguousarray(nl[:, i]).view(np.uint8).reshape(nb, 4)
        data[:, co + 8 * i + 4: co + 8 * i + 8] = np.ascontiguousarray(nw[:, i]).view(np.uint8).reshape(nb, 4)
    with open(path, "wb") as f:
        f.write(struct.pack(_VOC_HEAD, lay["alignment"], nb, wp, bs, fo, co, nb * bs, CV_32F, 4 * VOC_DIM, k))
        data.tofile(f)


def read_voctree(path):
    """-> dict(k, block_n [nb] uint16, node_desc [nb][k][128] float32, node_link [nb][k] uint32, node_weight [nb][k] float32,
    block_leaf [nb] uint16, block_parent [nb] uint32, layout): the arguments of write_voctree and of Context.voctree."""
    with open(path, "rb") as f:
        head = f.read(struct.calcsize(_VOC_HEAD))
        al, nb, wp, bs, fo, co, total, dtype, dsize, k = struct.unpack(_VOC_HEAD, head)
        if dtype != CV_32F or dsize != 4 * VOC_DIM:
            raise ValueError("voctree of descriptor type %d, %d bytes: only CV_32F, 512 bytes (SIFT)" % (dtype, dsize))
        if total < nb * bs or wp < dsize or co + 8 * k > bs or fo + k * wp > bs:
            raise ValueError("voctree header: the blocks do not fit")
        data = np.fromfile(f, dtype=np.uint8, count=total)
    if len(data) != total:
        raise ValueError("voctree file is short")
    data = data[:nb * bs].reshape(nb, bs)

    def col(a, b, dt):
        return np.ascontiguousarray(data[:, a:b]).view(dt)

    nd = np.stack([col(fo + i * wp, fo + i * wp + dsize, np.float32) for i in range(k)], axis=1)
    nl = np.concatenate([col(co + 8 * i, co + 8 * i + 4, np.uint32) for i in range(k)], axis=1)
    nw = np.concatenate([col(co + 8 * i + 4, co + 8 * i + 8, np.float32) for i in range(k)], axis=1)
    return dict(k=k, block_n=col(0, 2, np.uint16).reshape(nb), node_desc=nd, node_link=nl, node_weight=nw,
                block_leaf=col(2, 4, np.uint16).reshape(nb), block_parent=col(4, 8, np.uint32).reshape(nb),
                layout=dict(alignment=al, desc_size_bytes_wp=wp, feature_off_start=fo, child_off_start=co, block_size_bytes_wp=bs))


def write_bundle_out(path, cam_fk, cam_R, cam_t, points, views):
    """cam_fk [nc][3], cam_R [nc][9] row-major, cam_t [nc][3]; points [np][3]; views[p] = list of (camera, key, x, y)."""
    with open(path, "w") as ff:
        ff.write("# Bundle file v0.3\n")
        ff.write("%d %d\n" % (len(cam_t), len(points)))
        for i in range(len(cam_t)):
            ff.write("%.8f %.8f %.8f\n" % tuple(cam_fk[i]))
            ff.write(" ".join("%.8f" % v for v in np.asarray(cam_R[i]).reshape(9)) + "\n")
            ff.write("%.8f %.8f %.8f\n" % tuple(cam_t[i]))
        for p in range(len(points)):
            ff.write("%.8f %.8f %.8f " % tuple(points[p]))
            ff.write("255 255 255 ")
            ff.write("%d\n" % len(views[p]))
            for cam, key, x, y in views[p]:
                ff.write("%d %d %.8f %.8f\n" % (cam, key, float(int(x)), float(int(y))))   # int x = it1->second(0): truncation


def read_bundle_out(path):
    tok = open(path).read().split("\n")
    assert tok[0].startswith("# Bundle file")
    nc, npt = (int(v) for v in tok[1].split())
    fk, R, t = np.zeros((nc, 3)), np.zeros((nc, 9)), np.zeros((nc, 3))
    line = 2
    for i in range(nc):
        fk[i] = [float(v) for v in tok[line].split()]
        R[i] = [float(v) for v in tok[line + 1].split()]
        t[i] = [float(v) for v in tok[line + 2].split()]
        line += 3
    pts, views = np.zeros((npt, 3)), []
    for p in range(npt):
        v = tok[line].split()
        pts[p] = [float(x) for x in v[:3]]
        nv = int(v[6])
        line += 1
        vs = []
        for _ in range(nv):
            w = tok[line].split()
            vs.append((int(w[0]), int(w[1]), float(w[2]), float(w[3])))
            line += 1
        views.append(vs)
    return fk, R, t, pts, views


def write_openmvs(path, cams, points):
    """IncrementalSfM::SaveforOpenMVS (sfm_incremental.cc:1147-1245), sfm_openmvs.txt.
    cams: list of dict(image_path, f, R [9], t [3], id, px, py, w, h); points: list of dict(X [3], bad, views = [(cam index, x, y)]
    in std::map key order, x / y centred pixels).  Quirks kept: the image name is path[last '\\\\' : -1] (leading separator kept,
    last character dropped, :1171-1172); pixel coordinates are x + px truncated to int; the view COUNT is taken against the
    first view's camera size for every view (the counting loop never advances its camera iterator, :1203-1213) while the views
    actually written are tested against their own camera (:1234-1242)."""
    def pix(v, off):
        return int(v + off)   # int x = it1->second(0) + px_: double sum truncated toward zero

    with open(path, "w") as ff:
        ff.write("%d\n" % len(cams))
        for c in cams:
            p = c["image_path"]
            t = p.rfind("\\")
            ff.write(p[t:len(p) - 1] + "\n" if t >= 0 else p[-1:len(p) - 1] + "\n")   # npos: substr(npos, ..) would throw; empty here
            ff.write("%.8f\n" % c["f"])
            ff.write(" ".join("%.8f" % v for v in np.asarray(c["R"]).reshape(9)) + "\n")
            ff.write("%.8f %.8f %.8f\n" % tuple(c["t"]))
        goods = []
        for pt in points:
            if pt.get("bad"):
                goods.append(0)
                continue
            n = len(pt["views"])
            if n:
                c0 = cams[pt["views"][0][0]]
                for (_, x, y) in pt["views"]:
                    xi, yi = pix(x, c0["px"]), pix(y, c0["py"])
                    if xi < 0 or xi >= c0["w"] or yi < 0 or yi >= c0["h"]:
                        n -= 1
            goods.append(n)
        ff.write("%d\n" % sum(1 for pt, g in zip(points, goods) if not pt.get("bad") and g >= 2))
        for pt, g in zip(points, goods):
            if g < 2 or pt.get("bad"):
                continue
            ff.write("%.8f %.8f %.8f 255 255 255 %d\n" % (pt["X"][0], pt["X"][1], pt["X"][2], g))
            for (ci, x, y) in pt["views"]:
                c = cams[ci]
                xi, yi = pix(x, c["px"]), pix(y, c["py"])
                if not (xi < 0 or xi >= c["w"] or yi < 0 or yi >= c["h"]):
                    ff.write("%d %d %d\n" % (c["id"], xi, yi))


def _g(x):
    return format(float(x), ".20g")   # ofs.precision(20), default float field (sfm_incremental.cc:1472)


def write_temp_result(path, state):
    """IncrementalSfM::WriteTempResultOut (sfm_incremental.cc:1465-1573): the text checkpoint of a reconstruction.
    state = dict(cam_models=[dict(id, cam_maker, cam_model, w, h, f_mm, f, f_hyp, px, py, k1, k2, data[3], num_cams)],
                 cams=[dict(id_img, model_id, is_mutable, data[6], pts=[(key, point id)], visible_cams=[...])],
                 pts=[dict(id, is_mutable, is_bad_estimated, is_new_added, data[3], cams=[(key, id_img)], pts2d=[(key, x, y)],
                           key_new_obs, mse)], localize_fail_times=[...]); map-typed lists in ascending key order."""
    with open(path, "w") as f:
        f.write("%d\n" % len(state["cam_models"]))
        for m in state["cam_models"]:
            f.write("%d\n%s\n%s\n" % (m["id"], m["cam_maker"], m["cam_model"]))
            f.write("%d %d\n" % (m["w"], m["h"]))
            f.write(" ".join(_g(v) for v in (m["f_mm"], m["f"], m["f_hyp"], m["px"], m["py"], m["k1"], m["k2"], *m["data"][:3])) + "\n")
            f.write("%d\n" % m["num_cams"])
        f.write("%d\n" % len(state["cams"]))
        for c in state["cams"]:
            f.write("%d\n%d\n%d\n" % (c["id_img"], c["model_id"], int(bool(c["is_mutable"]))))
            f.write("".join(" " + _g(v) for v in c["data"][:6]) + "\n")
            f.write("%d\n" % len(c["pts"]))
            f.write("".join("%d %d " % (k, i) for k, i in c["pts"]) + "\n")
            f.write("%d\n" % len(c["visible_cams"]))
            f.write("".join("%d " % v for v in c["visible_cams"]) + "\n")
        f.write("%d\n" % len(state["pts"]))
        for p in state["pts"]:
            f.write("%d\n" % p["id"])
            f.write("%d %d %d\n" % (int(bool(p["is_mutable"])), int(bool(p["is_bad_estimated"])), int(bool(p["is_new_added"]))))
            f.write(" ".join(_g(v) for v in p["data"][:3]) + "\n")
            f.write("%d\n" % len(p["cams"]))
            f.write("".join("%d %d " % (k, i) for k, i in p["cams"]) + "\n")
            f.write("%d\n" % len(p["pts2d"]))
            f.write("".join("%d %s %s " % (k, _g(x), _g(y)) for k, x, y in p["pts2d"]) + "\n")
            f.write("%d\n" % p["key_new_obs"])
            f.write(_g(p["mse"]) + "\n")
        f.write("".join("%d " % v for v in state["localize_fail_times"]))


def read_temp_result(path, n_localize=None):
    """IncrementalSfM::ReadTempResultIn (sfm_incremental.cc:1575-1749), token by token like the `ifs >>` chain (the two
    camera strings are read with getline).  n_localize: how many trailing localisation counters to read (default: all)."""
    text = open(path).read()
    pos = 0

    def tok():
        nonlocal pos
        while pos < len(text) and text[pos].isspace():
            pos += 1
        start = pos
        while pos < len(text) and not text[pos].isspace():
            pos += 1
        return text[start:pos]

    def line():
        nonlocal pos
        end = text.find("\n", pos)
        end = len(text) if end < 0 else end
        s = text[pos:end]
        pos = min(len(text), end + 1)
        return s

    st = dict(cam_models=[], cams=[], pts=[], localize_fail_times=[])
    for _ in range(int(tok())):
        m = dict(id=int(tok()))
        line()                                  # rest of the id line (std::getline(ifs, temp))
        m["cam_maker"], m["cam_model"] = line(), line()
        m["w"], m["h"] = int(tok()), int(tok())
        vals = [float(tok()) for _ in range(10)]
        m.update(f_mm=vals[0], f=vals[1], f_hyp=vals[2], px=vals[3], py=vals[4], k1=vals[5], k2=vals[6], data=vals[7:10])
        m["num_cams"] = int(tok())
        st["cam_models"].append(m)
    for _ in range(int(tok())):
        c = dict(id_img=int(tok()), model_id=int(tok()), is_mutable=bool(int(tok())))
        c["data"] = [float(tok()) for _ in range(6)]
        c["pts"] = [(int(tok()), int(tok())) for _ in range(int(tok()))]
        c["visible_cams"] = [int(tok()) for _ in range(int(tok()))]
        st["cams"].append(c)
    for _ in range(int(tok())):
        p = dict(id=int(tok()), is_mutable=bool(int(tok())), is_bad_estimated=bool(int(tok())), is_new_added=bool(int(tok())))
        p["data"] = [float(tok()) for _ in range(3)]
        p["cams"] = [(int(tok()), int(tok())) for _ in range(int(tok()))]
        p["pts2d"] = [(int(tok()), float(tok()), float(tok())) for _ in range(int(tok()))]
        p["key_new_obs"] = int(tok())
        p["mse"] = float(tok())
        st["pts"].append(p)
    while n_localize is None or len(st["localize_fail_times"]) < n_localize:
        t = tok()
        if not t:
            break
        st["localize_fail_times"].append(int(t))
    return st
