"""What tests/test_cpu_paged.py and the GPU tests of the paged FP8 K/V cache share, restated here and NOT imported from the product
(include/qattn_paged.h is the contract): the literal address map of a pool, `gather` -- the contiguous image a table selects from a
pool, a chunk-level index copy --, the key-level page lookup with the three mutants the tables must expose, and the shared tables."""
import numpy as np
import torch

from tests import kvcache_cases as KC

KFRAG, VFRAG = KC.KFRAG, KC.VFRAG
FP8 = KC.FP8
NAN_BYTE = {"e4m3": 0x7F, "e5m2": 0x7E}
CAP = 1280                    # max_pages * page_size of every shared table
PAGE_SIZES = (64, 128, 256)
B, HKV = 3, 2


def chunk_start(p, h, c, Hkv, page_size, D):
    """byte at which chunk c of kv head h of page p starts in a pool (include/qattn_paged.h, literally)"""
    return ((p * Hkv + h) * (page_size // 64) + c) * 64 * D


def pool_bytes(num_pages, Hkv, page_size, D):
    return chunk_start(num_pages, 0, 0, Hkv, page_size, D)


def gather(pool, table, Hkv, page_size, D):
    """pool: flat uint8 (torch, any device), the KFRAG or VFRAG image of [num_pages, Hkv, page_size, D]; table: int [B, M] (in range).
    Returns the flat contiguous image of [B, Hkv, M page_size, D] in the same layout: chunk 64 m + c of (b, h) is chunk c of head h of
    page table[b][m].  Chunks are self-contained in both layouts, so the layout does not enter."""
    pc, CH = page_size // 64, 64 * D
    t = torch.as_tensor(table, dtype=torch.long, device=pool.device)
    Bt, M = t.shape
    return pool.view(-1, Hkv, pc, CH)[t].permute(0, 2, 1, 3, 4).reshape(Bt * Hkv * M * pc * CH).contiguous()


def gather_by_address(pool, table, Hkv, page_size, D):
    """`gather` once more, chunk by chunk through chunk_start on a numpy pool (slow: the check of the index copy above)"""
    pool = np.asarray(pool)
    pc, CH = page_size // 64, 64 * D
    Bt, M = len(table), len(table[0])
    out = np.zeros((Bt, Hkv, M * pc, CH), np.uint8)
    for b in range(Bt):
        for h in range(Hkv):
            for lc in range(M * pc):
                at = chunk_start(int(table[b][lc // pc]), h, lc % pc, Hkv, page_size, D)
                out[b, h, lc] = pool[at:at + CH]
    return out.reshape(-1)


# ---- the key-level lookup on a ROW-MAJOR pool [num_pages, Hkv, page_size, D] (numpy), and the mutants a test of the tables must expose
def lookup(table, b, j, page_size, mutant=None):
    """page and slot of key j of sequence b.  mutant: 'identity' ignores the table; 'row0' uses sequence 0's row for every sequence;
    'round-up' takes the page index from (j + 63) // page_size (clamped to the table's width)"""
    M = len(table[0])
    if mutant == "identity":
        return j // page_size, j % page_size
    if mutant == "row0":
        return int(table[0][j // page_size]), j % page_size
    if mutant == "round-up":
        return int(table[b][min((j + 63) // page_size, M - 1)]), j % page_size
    assert mutant is None
    return int(table[b][j // page_size]), j % page_size


def gather_rows(pool_rows, table, page_size, mutant=None):
    """row-major numpy pool [P, Hkv, page_size, D] -> [B, Hkv, M page_size, D] through `lookup` (pages beyond the pool: clamped)"""
    P = pool_rows.shape[0]
    Bt, M = len(table), len(table[0])
    j = np.arange(M * page_size)
    out = np.empty((Bt,) + pool_rows.shape[1:2] + (M * page_size,) + pool_rows.shape[3:], pool_rows.dtype)
    for b in range(Bt):
        ps = [lookup(table, b, int(x), page_size, mutant) for x in j]
        page = np.clip(np.array([p for p, _ in ps]), 0, P - 1)
        slot = np.array([s for _, s in ps])
        out[b] = pool_rows[page, :, slot].transpose(1, 0, 2)
    return out


# ---- the shared tables
def lens_sets(page_size):
    """four length triples that together hold every length of {0, 1, 63, 64, 65, ps - 1, ps, ps + 1, 1100, 1280}; each has a sequence long
    enough (>= 1100) for a FAST split to reach 1024 keys and for every mutant to show (sequence 0 is a short one: its row in place of a
    long sequence's is a large change)"""
    ps = page_size
    return [(ps + 1, 1100, 0), (63, 1280, ps - 1), (64, 1100, 1), (ps, 65, 1280)]


POISON = 2      # the pool page that holds NaN bytes in K and V


class Tables:
    """A pool geometry and a block table for B sequences of the given lengths (no page allocator of the product is involved):
      num_pages   B M + 2, M = CAP / page_size;  POISON is never handed out
      table       int32 numpy [B, M]: sequence b's first need_b = ceil(L_b / page_size) entries are distinct pages in shuffled order;
                  the two sequences with the most pages share their FIRST page (a common prefix); every entry behind need_b is POISON --
                  a valid index, so a kernel that reads one too many shows NaN, not a fault
      zeroed      the same with 0 in place of POISON"""

    def __init__(self, page_size, lens, seed=0, need=None):
        assert CAP % page_size == 0 and len(lens) == B
        self.page_size, self.lens = page_size, tuple(lens)
        self.M = CAP // page_size
        self.num_pages = B * self.M + 2
        rng = np.random.RandomState(1000 * page_size + seed)
        free = [p for p in rng.permutation(self.num_pages).tolist() if p != POISON]
        self.need = [-(-L // page_size) for L in lens] if need is None else list(need)
        self.table = np.full((B, self.M), POISON, np.int32)
        for b in range(B):
            for i in range(self.need[b]):
                self.table[b, i] = free.pop()
        # the common prefix page: the two sequences with the most pages share their first one (the longer one has more than one page, so
        # the two rows still differ)
        a, c = sorted(range(B), key=lambda b: -self.need[b])[:2]
        self.shared = need is None and self.need[c] > 0 and self.need[a] > 1
        self.sharers = (a, c) if self.shared else None
        if self.shared:
            self.table[c, 0] = self.table[a, 0]
        self.zeroed = np.where(np.arange(self.M)[None, :] < np.array(self.need)[:, None], self.table, 0).astype(np.int32)

    def check(self):
        """the properties the issue asks of the shared tables"""
        ident = np.arange(self.M)
        for b in range(B):
            assert not np.array_equal(self.table[b], ident), "a row is the identity"
            for c in range(b):
                assert not np.array_equal(self.table[b], self.table[c]), "two rows are equal"
            assert (self.table[b, self.need[b]:] == POISON).all() and (self.table[b, :self.need[b]] != POISON).all()
        used = [int(p) for b in range(B) for p in self.table[b, :self.need[b]]]
        assert len(used) - len(set(used)) == (1 if self.shared else 0), "pages are private, except the one shared prefix page"
        assert 0 <= self.table.min() and self.table.max() < self.num_pages


def shared_tables(page_size):
    return [Tables(page_size, lens, seed=i) for i, lens in enumerate(lens_sets(page_size))]


def random_rows(num_pages, page_size, D, fmt, seed, device="cpu"):
    """finite random fp8 rows of a pool [num_pages, HKV, page_size, D] as uint8 (torch), K and V"""
    g = torch.Generator().manual_seed(seed)
    mk = lambda: torch.randn(num_pages, HKV, page_size, D, generator=g).to(FP8[fmt]).view(torch.uint8).to(device)
    return mk(), mk()
