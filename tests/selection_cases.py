"""Input builders of the exhaustive selection tests (test_selection_cases.py on
the CPU, test_gpu_selection_exhaustive.py on the GPU): every 16-bit pattern as
a median and as a kept value of the trimmed mean, all 0/1 columns, structured
client orders, shared radix prefixes and every rounding boundary.

Plain functions of torch ops that run on any device; randomness comes from a
generator seeded per call on that device, so a case is the same on every run.
Columns are clients: a builder returns a (K, N) tensor, row i is client i."""
from __future__ import annotations

import torch

INF_BITS = {torch.bfloat16: 0x7F80, torch.float16: 0x7C00}
INT_OF = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def _gen(seed: int, device) -> torch.Generator:
    return torch.Generator(device=device).manual_seed(seed)


def from_bits(bits: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Integer bit patterns (any integer dtype, the low 16 or 32 bits count) as
    values of `dtype`."""
    if dtype == torch.float32:
        b = bits.to(torch.int64) & 0xFFFFFFFF
        return torch.where(b >= 1 << 31, b - (1 << 32), b).to(torch.int32).view(torch.float32)
    b = bits.to(torch.int32) & 0xFFFF
    return torch.where(b >= 1 << 15, b - (1 << 16), b).to(torch.int16).view(dtype)


def to_bits(x: torch.Tensor) -> torch.Tensor:
    """The raw bits of fp32 / bf16 / f16 values, unsigned, as int64."""
    x = x.contiguous()
    if x.dtype == torch.float32:
        return x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return x.view(torch.int16).to(torch.int64) & 0xFFFF


# ---- the 16-bit domain ----------------------------------------------------------

def ordered_patterns(dtype: torch.dtype) -> torch.Tensor:
    """The non-NaN bit patterns of bf16 / f16 in the kernels' total order,
    -inf ... -0, +0 ... +inf, as int32 (65,282 for bf16, 63,490 for f16)."""
    inf = INF_BITS[dtype]
    neg = torch.arange(0x8000 | inf, 0x8000 - 1, -1, dtype=torch.int32)
    pos = torch.arange(0, inf + 1, dtype=torch.int32)
    return torch.cat([neg, pos])


def nan_patterns(dtype: torch.dtype) -> torch.Tensor:
    """Every NaN bit pattern of bf16 / f16, both signs, as int32."""
    inf = INF_BITS[dtype]
    pos = torch.arange(inf + 1, 0x8000, dtype=torch.int32)
    return torch.cat([pos, pos | 0x8000])


def boundary_ranks(dtype: torch.dtype, K: int) -> torch.Tensor:
    """The ranks (indices into ordered_patterns) a test of K clients runs:
    all of them up to 1,024 clients; above that every 16th, plus 64 on either
    side of the -0 / +0 seam, of the subnormal / normal boundary of each sign
    and of the largest finite / inf of each sign."""
    inf = INF_BITS[dtype]
    R = 2 * (inf + 1)
    if K <= 1024:
        return torch.arange(R)
    min_normal = inf & -inf  # the exponent field's lowest bit: the smallest normal's pattern
    centres = [0, R - 1,  # -inf | largest finite, largest finite | +inf
               inf - min_normal, inf + 1 + min_normal,  # subnormal | normal, each sign
               inf]  # -0 | +0 (rank inf is -0, inf + 1 is +0)
    parts = [torch.arange(0, R, 16)] + [torch.arange(c - 64, c + 66) for c in centres]
    return torch.unique(torch.cat(parts).clamp(0, R - 1))


def _rand_ranks(lo: torch.Tensor, hi: torch.Tensor, rows: int, g: torch.Generator) -> torch.Tensor:
    """(rows, N) random integers in [lo, hi] per column."""
    u = torch.rand((rows, lo.numel()), generator=g, device=lo.device, dtype=torch.float64)
    span = (hi - lo + 1).to(torch.float64)
    return torch.minimum(lo + (u * span).floor().to(torch.int64), hi.expand(rows, -1))


def permute_columns(x: torch.Tensor, g: torch.Generator) -> torch.Tensor:
    """Every column of the (K, N) tensor in its own random client order."""
    order = torch.rand(x.shape, generator=g, device=x.device).argsort(dim=0)
    return torch.gather(x, 0, order)


def rank_columns(K: int, ranks: torch.Tensor, R: int, spread: str, seed: int, lo_count: "int | None" = None,
                 mid_count: int = 1) -> torch.Tensor:
    """(K, N) int64 ranks in [0, R): column j holds ranks[j] `mid_count`
    times from sorted position `lo_count` (default (K-1)//2) on; below it
    r-1, r-2 (clipped at 0) and random ranks <= r, above it r+1, r+2 (clipped)
    and random ranks >= r, from the whole range ("wide") or within K//4 of r
    ("narrow": shared high bits and many duplicates); then permuted per
    column."""
    assert spread in ("wide", "narrow")
    g = _gen(seed, ranks.device)
    r = ranks.to(torch.int64)
    N = r.numel()
    m = (K - 1) // 2 if lo_count is None else lo_count
    above = K - mid_count - m
    assert m >= 0 and above >= 0
    w = K // 4
    lo = torch.zeros_like(r) if spread == "wide" else (r - w).clamp(min=0)
    hi = torch.full_like(r, R - 1) if spread == "wide" else (r + w).clamp(max=R - 1)
    near_lo = torch.stack([(r - 1).clamp(min=0), (r - 2).clamp(min=0)])[:m]
    near_hi = torch.stack([(r + 1).clamp(max=R - 1), (r + 2).clamp(max=R - 1)])[:above]
    col = torch.cat([near_lo, _rand_ranks(lo, r, m - near_lo.shape[0], g),
                     r.expand(mid_count, N),
                     near_hi, _rand_ranks(r, hi, above - near_hi.shape[0], g)])
    assert col.shape == (K, N)
    return permute_columns(col, g)


def median_columns(dtype: torch.dtype, K: int, ranks: torch.Tensor, spread: str, seed: int) -> torch.Tensor:
    """(K, N) bf16 / f16 columns whose lower median is ordered_patterns(dtype)
    [ranks[j]] by construction (rank_columns)."""
    o = ordered_patterns(dtype).to(ranks.device)
    return from_bits(o[rank_columns(K, ranks, o.numel(), spread, seed)], dtype)


def nan_columns(dtype: torch.dtype, K: int, seed: int, device=None) -> "tuple[torch.Tensor, torch.Tensor]":
    """One column per NaN pattern of the dtype whose first NaN in client order
    is that pattern, with a different NaN at a later client; the rest finite.
    Returns the (K, N) columns and the (N,) expected bit patterns."""
    assert K >= 2
    pats = nan_patterns(dtype).to(device)
    n = pats.numel()
    g = _gen(seed, pats.device)
    o = ordered_patterns(dtype).to(pats.device)
    ranks = torch.randint(1, o.numel() - 1, (K, n), generator=g, device=pats.device)
    bits = o[ranks]
    j = torch.arange(n, device=pats.device)
    first = (j * 7) % (K - 1)
    later = first + 1 + (j * 13) % (K - 1 - first)
    bits[first, j] = pats
    bits[later, j] = pats[(j + 1) % n]
    return from_bits(bits, dtype), pats


def identity_columns(dtype: torch.dtype, K: int, trim: int, spread: str, seed: int, device=None
                     ) -> "tuple[torch.Tensor, torch.Tensor]":
    """Trimmed-mean columns for every interior rank r of the total order: the
    K - 2 trim kept positions all hold o[r], o[r-1] sits below and o[r+1] above
    them.  Returns the (K, N) columns and the (N,) kept value o[r]."""
    o = ordered_patterns(dtype).to(device)
    ranks = torch.arange(1, o.numel() - 1, device=o.device)
    col = rank_columns(K, ranks, o.numel(), spread, seed, lo_count=trim, mid_count=K - 2 * trim)
    return from_bits(o[col], dtype), from_bits(o[ranks], dtype)


def tie_columns(dtype: torch.dtype, seed: int, device=None) -> torch.Tensor:
    """(4, N) columns {-inf, a, succ(a), +inf}, permuted, for every adjacent
    pair of finite patterns of the total order (the -0 / +0 pair included):
    at trim 1 the mean of two neighbours is an exact tie of the final rounding
    wherever it does not fall on the coarser grid above a power of two."""
    o = ordered_patterns(dtype).to(device)
    R = o.numel()
    a = torch.arange(1, R - 2, device=o.device)
    col = torch.stack([torch.zeros_like(a), a, a + 1, torch.full_like(a, R - 1)])
    return from_bits(o[permute_columns(col, _gen(seed, o.device))], dtype)


# ---- 0/1 columns -----------------------------------------------------------------

def binary_columns(K: int, dtype: torch.dtype, device=None) -> "tuple[torch.Tensor, torch.Tensor]":
    """All 2^K columns of 0.0 / 1.0: client i of column c holds bit i of c.
    Returns the (K, 2^K) columns and the (2^K,) int64 number of ones."""
    c = torch.arange(1 << K, dtype=torch.int32, device=device)
    rows = torch.empty((K, 1 << K), dtype=dtype, device=device)
    ones = torch.zeros(1 << K, dtype=torch.int64, device=device)
    for i in range(K):
        b = (c >> i) & 1
        rows[i] = b
        ones += b
    return rows, ones


def binary_median(K: int, ones: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The lower median of 0/1 columns: 0 iff at least (K-1)//2 + 1 zeros."""
    m = (K - 1) // 2
    return (K - ones < m + 1).to(dtype)


def binary_trimmed_mean(K: int, trim: int, ones: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fedagg_trimmed_mean of 0/1 columns: the kept ranks hold
    clamp(ones - trim, 0, M) ones, whose fp32 sum is exact; one fp32 division
    by a tensor divisor, one rounding to the row dtype."""
    M = K - 2 * trim
    kept = (ones - trim).clamp(0, M).to(torch.float32)
    return (kept / torch.full((1,), float(M), dtype=torch.float32, device=ones.device)).to(dtype)


def bit_reversed_order(K: int) -> torch.Tensor:
    """The clients 0 .. K-1 ordered by their bit-reversed index."""
    nb = max(1, (K - 1).bit_length())
    rev = [int(format(i, f"0{nb}b")[::-1], 2) for i in range(K)]
    return torch.tensor(sorted(range(K), key=lambda i: rev[i]), dtype=torch.int64)


def _coprime(g: int, K: int) -> int:
    import math
    while math.gcd(g, K) != 1:
        g += 1
    return g


def placed_ones(K: int, ones: int, seed: int, device=None, n_random: int = 4096) -> torch.Tensor:
    """(K, N) bool: `ones` ones per column, placed as a cyclic contiguous run
    from every offset, at (offset + i g) mod K for g = 3, 5, 7 made coprime to
    K, at the first clients of the bit-reversed order, and at n_random seeded
    random places."""
    assert 0 <= ones <= K
    dev = torch.device(device) if device is not None else torch.device("cpu")
    i = torch.arange(K, device=dev)[:, None]
    off = torch.arange(K, device=dev)[None, :]
    parts = [((i - off) % K) < ones]
    for g0 in (3, 5, 7):
        g = _coprime(g0, K)
        ginv = pow(g, -1, K) if K > 1 else 0
        parts.append((((i - off) * ginv) % K) < ones)  # client (off + j g) mod K holds a one for j < ones
    br = torch.empty(K, dtype=torch.int64)
    br[bit_reversed_order(K)] = torch.arange(K)
    parts.append((br.to(dev) < ones)[:, None])
    rnd = torch.rand((K, n_random), generator=_gen(seed, dev), device=dev).argsort(dim=0)
    parts.append(rnd < ones)
    return torch.cat(parts, dim=1)


def decisive_median_ones(K: int) -> list:
    """The numbers of ones at which a 0/1 column's lower median flips: m + 1
    and m zeros."""
    m = (K - 1) // 2
    return sorted({K - (m + 1), K - m})


def decisive_trim_ones(K: int, trim: int) -> list:
    """The numbers of ones around both ends of the kept ranks."""
    return sorted({c for c in (trim - 1, trim, trim + 1, K - trim - 1, K - trim, K - trim + 1) if 0 <= c <= K})


# ---- distinct values in structured client orders ----------------------------------

def structured_orders(K: int, seed: int, device=None, n_random: int = 1024) -> torch.Tensor:
    """(K, N) int64: every column a permutation of 0 .. K-1 (the rank client
    i holds): ascending, descending, organ pipe and its inverse, even ranks
    then odd, bit reversal, rotations by every multiple of max(1, K // 64), and
    n_random random permutations."""
    dev = torch.device(device) if device is not None else torch.device("cpu")
    a = torch.arange(K)
    organ = torch.cat([a[0::2], a[1::2].flip(0)])  # rises through the even ranks, falls through the odd
    cols = [a, a.flip(0), organ, K - 1 - organ, torch.cat([a[0::2], a[1::2]]), bit_reversed_order(K)]
    cols += [torch.roll(a, s) for s in range(0, K, max(1, K // 64))]
    fixed = torch.stack(cols, dim=1).to(dev)
    rnd = torch.rand((K, n_random), generator=_gen(seed, dev), device=dev).argsort(dim=0)
    return torch.cat([fixed, rnd], dim=1)


def seam_band(dtype: torch.dtype, K: int, device=None) -> torch.Tensor:
    """K consecutive patterns of the total order centred on the -0 / +0 seam,
    ascending: K // 2 negative ones up to -0, then +0 on (fp32: denormals of
    both signs)."""
    j = torch.arange(K, dtype=torch.int64, device=device) - K // 2
    sign = 0x80000000 if dtype == torch.float32 else 0x8000
    return from_bits(torch.where(j < 0, sign | (-j - 1), j), dtype)


def one_band(dtype: torch.dtype, K: int, device=None) -> torch.Tensor:
    """K consecutive patterns centred on 1.0, ascending: distinct normal
    values in every dtype (quarter_values of more than 512 clients repeat in
    bf16)."""
    one = int(to_bits(torch.ones(1, dtype=dtype))[0])
    return from_bits(torch.arange(K, dtype=torch.int64, device=device) - K // 2 + one, dtype)


def quarter_values(dtype: torch.dtype, K: int, device=None) -> torch.Tensor:
    """(rank - K // 2) * 0.25, ascending: exact in fp32 for every K here."""
    return ((torch.arange(K, dtype=torch.float32, device=device) - K // 2) * 0.25).to(dtype)


VALUE_SETS = {"seam": seam_band, "quarter": quarter_values, "one": one_band}


# ---- radix-select prefixes (fp32) --------------------------------------------------

PREFIX_BASES = (0x3F800000, 0xBF800000, 0x00000000, 0x80000000, 0x42C80000)


def radix_prefix_columns(K: int, seed: int, device=None, per: int = 64) -> torch.Tensor:
    """(K, N) fp32 columns for the radix selects: per base (both signs,
    normals and the denormal range), only one byte of the pattern varying
    (byte 0, 1, 2: the rest shared), the same with the sign random too, all
    values equal but one, and two values with m, m + 1 and m + 2 copies of the
    smaller (m = (K-1)//2)."""
    dev = torch.device(device) if device is not None else torch.device("cpu")
    g = _gen(seed, dev)
    m = (K - 1) // 2
    half = per // 2
    parts = []
    for base in PREFIX_BASES:
        for byte in range(3):
            v = torch.randint(0, 256, (K, per), generator=g, device=dev)
            parts.append((base & ~(0xFF << 8 * byte)) | (v << 8 * byte))
    for base in PREFIX_BASES[0], PREFIX_BASES[2]:  # both sides of the sign boundary in one column
        for byte in range(3):
            v = torch.randint(0, 256, (K, half), generator=g, device=dev)
            s = torch.randint(0, 2, (K, half), generator=g, device=dev)
            parts.append((s << 31) | (base & ~(0xFF << 8 * byte)) | (v << 8 * byte))
    for base in PREFIX_BASES:
        b = base | 0x00400000  # away from zero, so that one pattern below stays on the same side
        for other in (b - 1, b + 1, b ^ 0x80000000):
            col = torch.full((K, half), b, dtype=torch.int64, device=dev)
            col[torch.randint(0, K, (half,), generator=g, device=dev), torch.arange(half, device=dev)] = other
            parts.append(col)
        small, large = (b, b + 1) if base < 0x80000000 else (b + 1, b)  # negative: the larger pattern is smaller
        for copies in (m, m + 1, m + 2):
            copies = min(copies, K)
            col = torch.where(torch.arange(K, device=dev)[:, None] < copies, small, large).expand(K, half)
            parts.append(permute_columns(col.contiguous(), g))
    return from_bits(torch.cat(parts, dim=1), torch.float32)


# ---- rounding boundaries ---------------------------------------------------------

def rounding_inputs(dtype: torch.dtype, device=None) -> torch.Tensor:
    """fp32 inputs of an fp32 -> bf16 / f16 rounding around every finite
    16-bit magnitude p and its successor (the largest finite one's successor
    is the power of two where inf begins), both signs: p itself, the midpoint
    (a tie), and the midpoint -1 and +1 fp32 ulp."""
    inf = INF_BITS[dtype]
    p = torch.arange(0, inf, dtype=torch.int32, device=device)
    if dtype == torch.bfloat16:
        exact = p.to(torch.int64) << 16
        mid = exact + 0x8000
    else:
        lo = from_bits(p, dtype).to(torch.float64)
        hi = from_bits(p + 1, dtype).to(torch.float64)
        hi[-1] = 65536.0  # where f16's exponent range ends: 65,520 is the tie into inf
        exact = to_bits(lo.to(torch.float32))
        midf = ((lo + hi) / 2).to(torch.float32)
        assert bool((midf.to(torch.float64) * 2 == lo + hi).all())  # the midpoints are exact in fp32
        mid = to_bits(midf)
    mag = torch.cat([exact, mid, mid - 1, mid + 1])
    return from_bits(torch.cat([mag, mag | 0x80000000]), torch.float32)


def nan_inputs(n: int, seed: int, device=None) -> torch.Tensor:
    """n fp32 NaNs of random payloads and signs, the quiet bit set or not;
    the first ones are the payload's extremes."""
    dev = torch.device(device) if device is not None else torch.device("cpu")
    g = _gen(seed, dev)
    man = torch.randint(1, 1 << 23, (n,), generator=g, device=dev)
    man[:6] = torch.tensor([1, 0x7FFFFF, 0x400000, 0x3FFFFF, 0x008000, 0x00FFFF], device=dev)
    sign = torch.randint(0, 2, (n,), generator=g, device=dev)
    sign[:6] = torch.tensor([0, 0, 0, 1, 1, 1], device=dev)
    return from_bits((sign << 31) | 0x7F800000 | man, torch.float32)


def all_patterns(dtype: torch.dtype, device=None) -> torch.Tensor:
    """All 65,536 patterns of bf16 / f16, NaNs included, in pattern order."""
    return from_bits(torch.arange(1 << 16, dtype=torch.int32, device=device), dtype)


WSUM_ONE_ROW_WEIGHTS = (1.0, 1 + 2.0 ** -8, 1 - 2.0 ** -9, 0.5, 2.0 ** -20, 3.0)
WSUM_TWO_ROW_CASES = tuple((shift, w) for shift in (1, 257) for w in ((0.5, 0.5), (1 + 2.0 ** -8, 2.0 ** -9)))
