"""Exact reference of the proposal ranking (abr_iod_amd/csrc/topk.hip): plain numpy, no GPU.

The library documents ONE order -- descending score, equal scores by ascending index -- for `topk_sigmoid` (RPN post-processor) and for
`abr_sort_scores_desc` (the score sort of `_C.nms`).  `torch.topk` leaves the members of a tie group undefined, so it cannot check that
contract; these two functions can:

  * `topk_ref(logits[N, nloc, ld], A, k)`: float64 1 / (1 + exp(-x)) over columns 0..A-1, flattened as loc * A + a, ranked by (score
    descending, index ascending) with np.lexsort; the first k indices and scores.  The rank is taken on the float64 value ROUNDED TO FLOAT32,
    which is what makes the certain saturations tie as they do in any float32 evaluation (+30, +inf -> 1.0f; -200, -inf -> 0.0f).  NaN
    scores rank first, as with torch.topk.
  * `sort_desc_ref(scores)`: the raw-key order on the uint32 view -- float order for every finite value, -0.0 strictly below +0.0, equal
    bit patterns by ascending index, +inf first and -inf last among the non-NaNs, NaNs at the ends by sign.

An index-exact comparison is only fair on logits whose ranking does not hang on the last bit of an `expf`.  The generators below therefore
draw from small value sets: multiples of 0.5 in [-8, 8] and the saturating specials.  Identical logits give identical keys (same
instruction sequence), distinct admitted logits differ in float32 sigmoid by thousands of ulps (tests/test_ranking_ref.py asserts at least
64 between neighbours of every set), so the reference order is the only defensible one."""
import numpy as np

HALVES = np.arange(-16, 17, dtype=np.float32) * np.float32(0.5)            # multiples of 0.5 in [-8, 8]
THREE = np.array([-1.0, 0.0, 1.0], np.float32)
ONE_BIN = np.arange(6, 17, dtype=np.float32) * np.float32(0.5)             # 3.0 .. 8.0: sigmoids in [0.9375, 1): one level-1 bin (key >> 20 == 0x3F7)
SPECIALS = np.array([30.0, -200.0, -np.inf, np.inf], np.float32)           # 1.0f, 0.0f, 0.0f, 1.0f
# value set of every generator the GPU tests use (test_ranking_ref.py checks the spacing of each)
VALUE_SETS = {"halves": HALVES, "three": THREE, "one_bin": ONE_BIN, "specials": np.concatenate([HALVES, SPECIALS]),
              "const": np.array([0.0], np.float32), "two": np.array([0.0, 2.0], np.float32)}


def sigmoid32(x):
    """float64 sigmoid rounded to float32"""
    with np.errstate(over="ignore"):
        return (1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))).astype(np.float32)


def draw(rng, name, shape, p=None):
    """logits of `shape` drawn from VALUE_SETS[name] (probabilities p)"""
    v = VALUE_SETS[name]
    return v[rng.choice(len(v), size=shape, p=p)]


def embed(rng, flat, A, ld):
    """flat [N, n] logits (n = nloc * A, anchor j = row j // A, column j % A) -> [N, nloc, ld] with the columns A.. filled with large decoys
    (+9 and NaN would win every ranking if the kernel read them)"""
    N, n = flat.shape
    y = np.where(rng.random((N, n // A, ld)) < 0.5, np.float32(9.0), np.float32(np.nan)).astype(np.float32)
    y[:, :, :A] = flat.reshape(N, n // A, A)
    return y


def topk_ref(logits, A, k):
    """-> (idx [N, k] int64, scores [N, k] float32)"""
    logits = np.asarray(logits)
    N = logits.shape[0]
    s = sigmoid32(logits[:, :, :A].reshape(N, -1))
    n = s.shape[1]
    rank = np.where(np.isnan(s), np.inf, s.astype(np.float64))
    idx = np.empty((N, k), np.int64)
    for i in range(N):
        idx[i] = np.lexsort((np.arange(n), -rank[i]))[:k]                   # last key is the primary one
    return idx, np.take_along_axis(s, idx, 1)


def sort_desc_ref(scores):
    """-> order [n] int64: descending in the order-preserving key of the bit pattern, equal patterns by ascending index"""
    b = np.ascontiguousarray(scores, np.float32).view(np.uint32).astype(np.int64)
    key = np.where(b >> 31, 0xFFFFFFFF - b, b + 0x80000000)                 # negative: every bit flipped; otherwise: the sign bit set
    return np.lexsort((np.arange(b.shape[0]), -key)).astype(np.int64)


# what the score sort must put in order: duplicates of both signs, denormals, zeros of both signs, infinities, NaNs of both signs (the NaNs
# from their bit patterns: a conversion through float64 would quieten the signalling one)
SORT_ZOO = np.concatenate([
    np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 3.5, -7.25, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.17549435e-38, 3.4028235e38, -3.4028235e38,
              np.inf, -np.inf], np.float32),
    np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32).view(np.float32)])


def sort_zoo(rng, n, specials=True):
    """n scores: half of them from a grid of halves (long runs of ties, both signs), the rest from SORT_ZOO.  specials=False: no signed
    zeros and no NaNs (SORT_ZOO without them, the grid's zeros become 0.25) -- the inputs on which torch.sort(stable) is a second opinion"""
    grid = np.round(rng.standard_normal(n).astype(np.float32) * 2) / np.float32(2)
    zoo = SORT_ZOO if specials else SORT_ZOO[2:17]
    s = np.where(rng.random(n) < 0.5, grid, zoo[rng.integers(0, len(zoo), n)]).astype(np.float32)
    if not specials:
        s[s == 0] = np.float32(0.25)
    return s
