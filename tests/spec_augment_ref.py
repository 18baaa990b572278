"""Helper, not a test: cfm_spec_augment (include/cfm.h) restated in numpy integers, next to a restatement of the reference's processor.spec_aug loop
(src/processor.py:151-172) that takes its random integers from a list instead of the `random` module -- so that a test can show the two agree on
the same draws.

  cfm_hash32(s, i): h = (i * 0x9E3779B1) ^ s;  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16      (uint32)
  r(b, k) = hash32(hash32(seed, ids[b]), k);   U[0, N - 1] = (uint64(r) * N) >> 32
  mask m (time masks first) draws its start with k = 2 m from U[0, T - 1] (time) or U[0, F - 1] (frequency) and its length with k = 2 m + 1 from
  1 + U[0, max - 1]; end = min(T or F, start + length).  T == 0 or F == 0: no masks, (0, 0) in the table.
  A training step enters the seed as seed + 0x9E3779B1 * step mod 2^32."""
import numpy as np

GOLDEN = 0x9E3779B1
M32 = 0xFFFFFFFF

# the cases of tests/test_augment_gpu.py, here so that tests/test_augment_cpu.py can check on the host that they exercise what they are meant to
SEED, STEPS = 20261020, (3, 4)
LENGTHS, T_MAX, IDS = [0, 1, 7, 50, 64], 64, [7, 0xFFFFFFF0, 2, 123456789, 4]
FEATURES, COUNTS, MAX_T, MAX_F = (80, 5), ((2, 2), (0, 3), (3, 0)), 50, 50


def hash32(seed, idx):
    """cfm_hash32 on uint32 arrays (or scalars), wrapping as the device does."""
    seed, idx = np.asarray(seed, dtype=np.uint64), np.asarray(idx, dtype=np.uint64)
    h = ((idx * GOLDEN) & M32) ^ seed
    h ^= h >> np.uint64(16)
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> np.uint64(13)
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def uniform(r, N):
    """U[0, N - 1] from 32 random bits: multiply-high."""
    return ((np.asarray(r, dtype=np.uint64) * np.uint64(N)) >> np.uint64(32)).astype(np.int64)


def step_seed(seed, step):
    return (int(seed) + GOLDEN * int(step)) & M32


def draws(seed, item_id, T, F, num_t_mask, num_f_mask, max_t, max_f):
    """The list of integers the reference's loop would take from random.randint, in its order: per mask (start, length)."""
    item = hash32(seed, int(item_id) & M32)
    out = []
    for m in range(num_t_mask + num_f_mask):
        N, most = (T, max_t) if m < num_t_mask else (F, max_f)
        out.append(int(uniform(hash32(item, 2 * m), N)))
        out.append(1 + int(uniform(hash32(item, 2 * m + 1), most)))
    return out


def mask_table(seed, ids, lengths, T_max, F, num_t_mask, num_f_mask, max_t, max_f):
    """int32 [B, num_t_mask + num_f_mask, 2]: (start, end) of every mask, straight from the definition."""
    B, nm = len(lengths), num_t_mask + num_f_mask
    table = np.zeros((B, nm, 2), np.int32)
    for b in range(B):
        T = min(max(int(lengths[b]), 0), T_max)
        if T == 0 or F == 0:
            continue
        d = draws(seed, ids[b], T, F, num_t_mask, num_f_mask, max_t, max_f)
        for m in range(nm):
            N = T if m < num_t_mask else F
            table[b, m] = (d[2 * m], min(N, d[2 * m] + d[2 * m + 1]))
    return table


def apply_table(feats, lengths, table, num_t_mask):
    """A copy of feats [B, T_max, F] with the table's masks written as +0.0: time masks zero rows, frequency masks columns of rows [0, T)."""
    y = np.array(feats, copy=True)
    for b in range(y.shape[0]):
        T = min(max(int(lengths[b]), 0), y.shape[1])
        for m, (start, end) in enumerate(table[b]):
            if m < num_t_mask:
                y[b, start:end, :] = 0.0
            else:
                y[b, :T, start:end] = 0.0
    return y


def reference_loop(x, num_t_mask, num_f_mask, max_t, max_f, randint):
    """processor.spec_aug's body for one sample x [frames, freq], with randint(a, b) handed in (the reference uses random.randint): returns the
    masked copy and the (start, end) pairs in the order they were drawn."""
    y = np.array(x, copy=True)
    pairs = []
    for axis, count, most in ((0, num_t_mask, max_t), (1, num_f_mask, max_f)):      # all time masks, then all frequency masks
        size = y.shape[axis]
        for _ in range(count):
            start = randint(0, size - 1)                                          # both ends inclusive, as random.randint
            end = min(size, start + randint(1, most))
            if axis == 0:
                y[start:end, :] = 0
            else:
                y[:, start:end] = 0
            pairs.append((start, end))
    return y, pairs


def replay(values):
    """A randint that hands out pre-drawn integers and checks each lies in the range the loop asks for."""
    it = iter(values)

    def randint(a, b):
        v = next(it)
        assert a <= v <= b, (a, v, b)
        return v
    return randint
