"""CPU: the additive entry points of the dead-tile skipping (include/nerf_hip.h) -- the size of the live-tile list, the argument
checks of the *_live forms -- and a numpy emulation of the list's layout (csrc/launchers.h, LiveTiles) with the arithmetic the
weight-gradient GEMM uses to find its chunk's slice: every stage of the sparse ring must address a tile the dense ring addresses."""
import numpy as np

import nerf_pytorch_amd as npa

HEADER = 4


def layout(n_tiles):
    n_words = (n_tiles + 31) // 32
    bitmap = HEADER + n_tiles
    prefix = bitmap + n_words
    total = (prefix + n_words + 1 + 3) // 4 * 4
    return n_words, bitmap, prefix, total


def test_live_list_size_and_argument_errors():
    L = npa.hip_backend.lib()
    for n, S in ((4096, 192), (4096, 64), (37, 5), (5, 3), (1, 1), (333, 77)):
        T = (n * S + 31) // 32
        assert L.nerf_live_tiles_words(n, S) == layout(T)[3]
        assert L.nerf_live_tiles_words(n, S) >= 4 + T                   # count word(s) + one word per tile
    assert L.nerf_live_tiles_words(0, 64) == 0 and L.nerf_live_tiles_words(4, -1) == 0
    assert L.nerf_bwd_skip_dead() in (0, 1)
    assert L.nerf_abi_version() == 10                                   # additive: the version stands
    # the *_live forms check what the dense forms check ...
    assert L.nerf_field_dgrad_split_live(None, None, None, 4, 4, None, 1, None, None) == -1 and b"null pointer" in L.nerf_last_error()
    assert L.nerf_field_dgrad_split_live(0x1000, 0x2000, 0x3000, 4, 4, 0x4000, 2, 0x5000, None) == -1       # split 2 is not a training split
    assert L.nerf_field_dgrad_split_live(0x1000, 0x2000, 0x3000, 4, 4, 0x4000, 1, 0x5004, None) == -1 and b"aligned" in L.nerf_last_error()
    assert L.nerf_field_wgrad_phase_live(None, None, None, 4, 4, None, None, 0, 5, 7, None, None, None) == -1
    assert b"null pointer" in L.nerf_last_error()
    assert L.nerf_field_wgrad_phase_live(0x1000, 0x2000, 0x3000, 4, 4, 0x4000, 0x5000, 0, 7, 7, 0x6000, 0x7000, None) == -1    # datapath 7
    assert L.nerf_field_wgrad_phase_live(0x1000, 0x2000, 0x3000, 4, 4, 0x4000, 0x5000, 0, 5, 7, 0x6000, 0x7004, None) == -1
    assert b"aligned" in L.nerf_last_error()
    # ... and the fp32 datapath has no sparse form
    assert L.nerf_field_wgrad_phase_live(0x1000, 0x2000, 0x3000, 4, 4, 0x4000, 0x5000, 0, 0, 7, None, 0x7000, None) == -1
    assert b"no sparse form" in L.nerf_last_error()


def wgrad_chunks(P, n_jobs=12):
    n = 256 // n_jobs
    n = max(1, min(n, (P + 255) // 256))
    pts = (P + n - 1) // n
    pts = (pts + 31) // 32 * 32
    return pts, (P + pts - 1) // pts


def emulate_scan(alive):
    """what delta_amax_kernel<true> + live_scan_kernel leave in the list buffer, from the per-tile flags"""
    T = len(alive)
    n_words, bitmap, prefix, total = layout(T)
    buf = np.full(total, 0xdeadbeef, dtype=np.uint64)
    bits = np.zeros(n_words * 32, dtype=np.uint64)
    bits[:T] = alive
    words = (bits.reshape(n_words, 32) << np.arange(32, dtype=np.uint64)).sum(1)
    buf[bitmap:bitmap + n_words] = words
    pos = 0
    for w in range(n_words):
        buf[prefix + w] = pos
        for b in range(32):
            if (int(words[w]) >> b) & 1:
                buf[HEADER + pos] = 32 * w + b
                pos += 1
    buf[prefix + n_words] = pos
    buf[0], buf[1], buf[2], buf[3] = pos, T, 0, 0
    return buf


def test_chunk_slices_of_the_list_address_dense_tiles():
    rng = np.random.default_rng(0)
    for P in (4096 * 64, 4096 * 192, 129 * 64, 37 * 5, 333 * 77, 1, 31, 32, 33, 1024, 1025):
        T = (P + 31) // 32
        n_words, bitmap, prefix, total = layout(T)
        pts, n_chunks = wgrad_chunks(P)
        assert pts % 32 == 0
        for pattern in ("random", "none", "all", "alternate", "runs"):
            alive = {"random": rng.random(T) < 0.5, "none": np.zeros(T, bool), "all": np.ones(T, bool),
                     "alternate": np.arange(T) % 2 == 0, "runs": (np.arange(T) // 13) % 2 == 1}[pattern]
            buf = emulate_scan(alive.astype(np.uint64))
            want = np.nonzero(alive)[0]
            count = int(buf[0])
            assert count == len(want) and np.array_equal(buf[HEADER:HEADER + count], want)

            def before(t):
                w, r = t >> 5, t & 31
                c = int(buf[prefix + w])
                assert prefix + w < total
                if r:
                    assert w < n_words
                    c += bin(int(buf[bitmap + w]) & ((1 << r) - 1)).count("1")
                return c

            seen = []
            for chunk in range(n_chunks):
                p_begin, p_end = chunk * pts, min((chunk + 1) * pts, P)
                tile0, n_tiles = p_begin >> 5, (p_end - p_begin + 31) // 32
                lo = before(tile0)
                n_st = before(tile0 + n_tiles) - lo
                for st in range(n_st):
                    assert HEADER + lo + st + 1 < total                 # the look-ahead word of issue() is inside the buffer
                    t = int(buf[HEADER + lo + st]) - tile0
                    assert 0 <= t < n_tiles                             # a tile of THIS chunk: the source offsets are dense ones
                    seen.append(tile0 + t)
                assert HEADER + lo < total                              # t_next's first read, also for an empty slice
            assert np.array_equal(np.array(seen, dtype=np.int64), want)     # every live tile exactly once, ascending
