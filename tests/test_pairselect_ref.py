"""tests/pairselect_ref.py against cases worked by hand, and the three file formats of the pair selection byte for byte."""
import numpy as np

from metricsfm_amd import featurefiles, matchfiles, pairsel
from tests import pairselect_ref as ref


def test_first_and_last_group_are_never_inverted():
    # groups 3 | 5 | 8 | 9, all single: g0 = 3 and gm = 9 stay out
    assert ref.keep_unique_vector([8, 3, 9, 5]) == [5, 8]
    assert ref.keep_unique_vector([4]) == []
    assert ref.keep_unique_vector([4, 6]) == []


def test_a_word_seen_twice_is_not_inverted():
    # groups 1 | 2 2 | 4 | 7 7 7 | 8 | 9
    assert ref.keep_unique_vector([7, 2, 9, 4, 7, 1, 2, 8, 7]) == [4, 8]


def test_table_entry_iff_the_preceding_group_is_a_singleton():
    #  feature : 0  1  2  3  4  5  6  7  8
    #  word    : 7  2  9  4  7  1  2  8  7
    #  groups  : g0 = 1 (f5) | g1 = 2 (f1, f6) | g2 = 4 (f3) | g3 = 7 (f0, f4, f8) | g4 = 8 (f7) | g5 = 9 (f2)
    #  g2: g1 is a pair -> no.  g3: g2 single -> yes, lowest feature 0 (its own size does not matter).  g4: g3 is a triple -> no.
    #  g5: g4 single -> yes (the last group counts here).
    w = [7, 2, 9, 4, 7, 1, 2, 8, 7]
    assert ref.keep_unique_idx_vector(w) == [0, 2]
    assert ref.pt_word_map(w) == {7: 0, 9: 2}


def test_g0_and_g1_are_never_in_the_table():
    # all single: 1 (f0) | 2 (f1) | 3 (f2) | 4 (f3): g0 opens nothing, g1 = 2 follows the first group, which is never unique
    assert ref.pt_word_map([1, 2, 3, 4]) == {3: 2, 4: 3}
    assert ref.pt_word_map([5, 6]) == {}
    assert ref.pt_word_map(None) == {} and ref.pt_word_map([]) == {}


def _image_with(word, num_words):
    return [0, word, num_words]   # the word as a single feature, neither the first nor the last group


def test_stop_size_and_small_vocabularies():
    num_words = 300   # th_bin_size 3
    words = [_image_with(10, num_words) for _ in range(4)]
    assert not ref.similarity_graph_inv_file(words, num_words).any()   # a bin of num_words / 100 + 1 = 4 images is emptied
    words = [_image_with(10, num_words) for _ in range(3)] + [_image_with(30, num_words)]
    S = ref.similarity_graph_inv_file(words, num_words)   # a bin of exactly num_words / 100 = 3 counts
    want = np.zeros((4, 4), np.int32)
    want[:3, :3] = 1 - np.eye(3, dtype=np.int32)
    assert (S == want).all() and S.dtype == np.int32
    inv = ref.generate_inverted_file(words, num_words)   # id num_words is always the last group: it never reaches the table
    assert inv[10] == [0, 1, 2] and inv[30] == [3] and inv[0] == [] and len(inv) == num_words
    words = [_image_with(10, 99) for _ in range(3)]
    assert not ref.similarity_graph_inv_file(words, 99).any()    # num_words < 100: a stop size of 0 empties every bin


def test_tie_order_of_the_ranking():
    S = np.array([[0, 2, 5, 2, 0],
                  [2, 0, 0, 0, 0],
                  [5, 0, 0, 1, 1],
                  [2, 0, 1, 0, 1],
                  [0, 0, 1, 1, 0]])
    assert ref.hypotheses(S, 0, 4) == ([2, 1, 3, 4], [5, 2, 2, 0])
    assert ref.hypotheses(S, 1, 3) == ([0, 2, 3], [2, 0, 0])
    assert ref.hypotheses(S, 4, 2) == ([2, 3], [1, 1])


def test_the_rule_for_k():
    assert [ref.th_num_match(n) for n in (12, 2500, 6000)] == [11, 250, 500]
    assert [pairsel.rule_k(n) for n in (12, 2500, 6000)] == [11, 250, 500]
    assert ref.th_num_match(201) == 200 and ref.th_num_match(2000) == 200


def test_join_is_in_ascending_word_order():
    assert ref.join({9: 0, 3: 4, 5: 1}, {5: 7, 9: 2, 4: 0}) == [(1, 7), (0, 2)]


def test_words_file_round_trip(tmp_path):
    fold = str(tmp_path)
    ids, wts, wid = [3, 9, 11], [0.25, 0.5, 0.125], [9, 3, 3, 11, 9]
    featurefiles.write_words(fold, 0, ids, wts, 4095, wid)
    raw = open(featurefiles.words_file(fold, 0), "rb").read()
    want = (np.array([3, 3, 9, 11], "<i4").tobytes() + np.array(wts, "<f4").tobytes() + np.array([4095, 5], "<i4").tobytes()
            + np.array(wid, "<i4").tobytes())
    assert raw == want
    a, b, m, c = featurefiles.read_words(fold, 0)
    assert list(a) == ids and list(b) == wts and m == 4095 and list(c) == wid
    featurefiles.write_words(fold, 1, a, b, m, c)
    assert open(featurefiles.words_file(fold, 1), "rb").read() == raw
    featurefiles.write_words(fold, 2, None, None, 0, None)   # an image without words: an empty file
    assert open(featurefiles.words_file(fold, 2), "rb").read() == b""
    assert featurefiles.read_words(fold, 2) == (None, None, None, None)


def test_init_match_graph_round_trip(tmp_path):
    fold = str(tmp_path)
    graph = [[1, 2], [], [0]]
    matchfiles.write_init_match_graph(fold, graph)
    raw = open(tmp_path / "init_match_graph.txt", "rb").read()
    assert raw == b"3\n2\n2 1 2 \n0 \n1 0 \n"
    assert matchfiles.read_init_match_graph(fold) == (graph, 2)
    matchfiles.write_init_match_graph(fold, graph, id_last=1)
    assert open(tmp_path / "init_match_graph.txt", "rb").read() == b"3\n1\n2 1 2 \n0 \n1 0 \n"
    assert matchfiles.read_init_match_graph(fold) == (graph, 1)


def test_similarity_graph_round_trip(tmp_path):
    fold = str(tmp_path)
    S = np.array([[0, 12, 3], [12, 0, 0], [3, 0, 0]], np.int32)
    matchfiles.write_similarity_graph(fold, S)
    raw = open(tmp_path / "similarity_graph.txt", "rb").read()
    assert raw == b"3\n0 12 3 \n12 0 0 \n3 0 0 \n"
    back = matchfiles.read_similarity_graph(fold)
    assert back.dtype == np.float32 and (back == S).all()
    matchfiles.write_similarity_graph(fold, back)
    assert open(tmp_path / "similarity_graph.txt", "rb").read() == raw
