"""The planted scenes of the pair-selection tests (tests/test_gpu_pairselect.py, tests/pairselect_host_check.cc's runner)."""
import numpy as np

from metricsfm_amd import scene

NUM_WORDS = 500          # stop size 5 (similarity_graph.cc:109)
NO_WORDS_IMAGE = 7
STRANGER = 11            # none of its features carries its point's word: what it shares with others is chance
RANDOM_PAIR = (0, 11)    # share 40 planted words on features at random positions: joined, but no epipolar geometry
WORD_IN_6, WORD_IN_5 = 412, 414


def planted_scene():
    """12 aerial images of about 400 features.  Words: a 3-D point's id for its observations (0 .. 299), distractors random in
    [200, 410] (so they repeat, and collide with point words); ids from 411 on are planted:
      412 once in images 1 .. 6 (a bin of 6 > 5: emptied), 414 once in images 1 .. 5 (a bin of 5: counts), 416 once in images
      1 .. 6 (so that neither is the last group); image 0 holds 419 .. 499 once each and image 11 the even ids 418 .. 498, so
      the tables of 0 and 11 share exactly the 40 even ids 420 .. 498, on distractor features; image 2 repeats the word of one of
      its points on a distractor; image 7 has no words; image 11 draws the words of ALL its features like distractors, so no
      pair with it has epipolar geometry behind its joined matches.
    -> dict(n_features, words (list, None for image 7), num_words, keypoints [sum][2] float32, feat_off, scene)"""
    sc = scene.make_aerial_scene(n_cams=12, n_points=300, seed=scene.SEED_BASE + 0x5e1, name="pairsel")
    sc = scene.add_features(sc, 400)
    rng = np.random.Generator(np.random.PCG64(scene.SEED_BASE + 0x5e2))
    words = []
    for c in range(sc.n_cams):
        fp = sc.feat_point[c]
        w = np.where(fp >= 0, fp, 0).astype(np.int32)
        dis = np.flatnonzero(fp < 0)
        if c == STRANGER:
            dis = np.arange(len(w))
        w[dis] = rng.integers(200, 411, size=dis.size)
        free = list(rng.permutation(dis))   # distractor features that take the plants

        def plant(ids):
            for wid in ids:
                w[free.pop()] = wid

        if 1 <= c <= 6:
            plant([WORD_IN_6, 416])
        if 1 <= c <= 5:
            plant([WORD_IN_5])
        if c == RANDOM_PAIR[0]:
            plant(range(419, 500))
        if c == RANDOM_PAIR[1]:
            plant(range(418, 500, 2))
        if c == 2:
            w[free.pop()] = w[np.flatnonzero(fp >= 0)[5]]
        words.append(w)
    words[NO_WORDS_IMAGE] = None
    n_features = np.array([len(k) for k in sc.kp_xy], dtype=np.int32)
    feat_off = np.concatenate([[0], np.cumsum(n_features)]).astype(np.int64)
    return dict(n_features=n_features, words=words, num_words=NUM_WORDS, keypoints=np.concatenate(sc.kp_xy).astype(np.float32),
                feat_off=feat_off, scene=sc)


def long_tables():
    """Two images of 5 000 features with 4 500 shared words and a third of 70 000 features: tables far longer than one
    256-entry piece of a workgroup.  Every word occurs once per image, so (but for g0 and g1) every word is a table entry."""
    rng = np.random.Generator(np.random.PCG64(scene.SEED_BASE + 0x5e3))
    num_words = 200000
    pool = rng.permutation(num_words)
    a = pool[:5000]
    b = np.concatenate([a[:4500], pool[5000:5500]])
    c = pool[2000:72000]
    words = [rng.permutation(x).astype(np.int32) for x in (a, b, c)]
    n_features = np.array([len(w) for w in words], dtype=np.int32)
    kp = rng.uniform(-2000, 2000, size=(int(n_features.sum()), 2)).astype(np.float32)
    feat_off = np.concatenate([[0], np.cumsum(n_features)]).astype(np.int64)
    return dict(n_features=n_features, words=words, num_words=num_words, keypoints=kp, feat_off=feat_off)


def sparse_images(n, num_words, shared, seed):
    """n images of a few features: word 0, one private word each, the `shared` words in the images listed for them, and
    num_words itself.  shared: dict word -> images.  Tiny tables; what it exercises is bins and rankings over many images."""
    rng = np.random.Generator(np.random.PCG64(scene.SEED_BASE + seed))
    private = rng.permutation(np.arange(1000, num_words))[:n]
    words = [[0, int(private[i]), num_words] for i in range(n)]
    for w, imgs in shared.items():
        for i in imgs:
            words[i].append(w)
    words = [rng.permutation(np.array(w, np.int32)) for w in words]
    n_features = np.array([len(w) for w in words], dtype=np.int32)
    kp = rng.uniform(-2000, 2000, size=(int(n_features.sum()), 2)).astype(np.float32)
    return dict(n_features=n_features, words=words, num_words=num_words, keypoints=kp)


def host_check_command(exe, args_only=False):
    """The compiler call for tests/pairselect_host_check.cc against this tree's library; args_only: the argument checks
    alone, which need neither library nor device, built with the host sanitizers."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "pairselect_host_check.cc")
    if args_only:
        return ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                "-DPAIRSELECT_ARGS_ONLY", "-I", os.path.join(root, "include"), src, "-o", str(exe)]
    lib = os.path.join(root, "metricsfm_amd")
    return ["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(root, "host"), "-I", os.path.join(root, "include"), src,
            os.path.join(root, "host", "objectsfm.cc"), "-o", str(exe), "-L" + lib, "-lmsfm", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib"]


def write_image_set(path, d, rows_per_call, max_hypotheses=0):
    """A scene in the byte layout tests/pairselect_host_check.cc reads."""
    with open(path, "wb") as fh:
        n = len(d["n_features"])
        has = [w is not None for w in d["words"]]
        np.array([n, d["num_words"], rows_per_call, max_hypotheses], np.int32).tofile(fh)
        np.asarray(d["n_features"], np.int32).tofile(fh)
        np.array(has, np.int32).tofile(fh)
        for k in range(n):
            (np.asarray(d["words"][k], np.int32) if has[k] else np.zeros(d["n_features"][k], np.int32)).tofile(fh)
        np.ascontiguousarray(d["keypoints"], np.float32).tofile(fh)


def read_host_result(path, n):
    """What pairselect_host_check.cc wrote: dict of hyp_img, n_init, n_inliers, verdict [n][K]."""
    raw = np.fromfile(path, np.int32)
    K = int(raw[0])
    a = raw[1:].reshape(n, 4, K)
    return dict(hyp_img=a[:, 0], n_init=a[:, 1], n_inliers=a[:, 2], verdict=a[:, 3].astype(np.uint8))
