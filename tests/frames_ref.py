"""The frame walk of the decoders behind a slicer (TSBK, P25 voice, EDACS) restated: the plain sequential rule over the hits,
one at a time -- what the kernels' 64-hit trips (radiocapture-rf_amd/csrc/item_wave.hpp, frame_walk) must come to.  A stage's
constants, in symbols: sync, the sync word's length (a hit's k is its last symbol); accept, how far behind the last accepted hit
the next one is; decide, how much of a frame must be in whole words before it is decided; longest, the longest frame;
per_word, symbols per word of the slicer's ring; cut, whether the next accepted hit cuts the frame short."""


def frame_walk(k, launches, st, first_hit=0, word_cap=None, hit_cap=None, *, sync, accept, decide, longest, per_word, cut):
    """yields (i, s, fd) for every decided frame the word ring still holds: hit i's frame starts at symbol s and has fd symbols.
    k: the hits' k from the slicer's start; launches: [(n_words, n_hits)] after each block; st: a dict whose n_frames and n_lost
    count the decided frames and what left the two rings unexamined; first_hit: the slicer's n_hits when the stage was attached;
    word_cap / hit_cap: the rings' capacities (None: nothing is ever overwritten)"""
    i, k_last = first_hit, None
    for n_words, n_hits in launches:
        if hit_cap and i < n_hits - hit_cap:
            st["n_lost"] += n_hits - hit_cap - i
            i = n_hits - hit_cap
        while i < n_hits:
            if k_last is not None and k[i] < k_last + accept:
                i += 1
                continue
            s = k[i] - (sync - 1)
            if per_word * n_words < s + decide:
                break
            later = [v for v in k[i + 1:n_hits] if v >= k[i] + accept] if cut else []
            fd = min(longest, later[0] - k[i]) if later else longest
            k_last = k[i]
            st["n_frames"] += 1
            i += 1
            if word_cap and s // per_word < n_words - word_cap:
                st["n_lost"] += 1
                continue
            yield i - 1, s, fd
