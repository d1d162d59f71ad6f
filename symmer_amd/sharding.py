"""The multi-rank algorithms, as functions of a communicator (``symmer_amd/parallel.py``): this rank's block of the sharded
commutation table and product, and the product + cleanup across ranks in two forms — the outer index in contiguous blocks
(``sharded_mul_cleanup``) and the pairs partitioned by a GF(2)-linear class of their product row (``hash_partitioned_mul_cleanup``).

Every algorithm has a host form (NumPy arrays in and out, the per-rank kernels injected, so that the CPU tests run the plumbing
with checker kernels) and a device form (``*_dev``: DeviceOps in and out, nothing but counts and pair indices on the host).  What the
two forms of an algorithm share is written once: the ragged all-gather (:func:`gather_ragged` / :func:`gather_ragged_dev`), the
class-bit rule and the walk over a rank's sub-products (:func:`class_bits`, :func:`owned_subproducts`), the ``stats`` record.
"""
import numpy as np
from . import kernels, packing
from .parallel import shard_bounds


# ---- ragged all-gather: every rank contributes a different number of rows ----------------------------------------------------------
def gather_ragged(comm, *arrays):
    """Host arrays with a common leading length that differs between the ranks -> the same arrays of ALL ranks, concatenated in rank
    order, on every rank: the counts go over the control plane, every array is padded to the longest, gathered, and the
    ``counts[r]`` leading rows of every rank are kept."""
    n_loc = arrays[0].shape[0]
    counts = np.frombuffer(comm.control.allgather(np.int64(n_loc).tobytes()), dtype=np.int64)
    ts = max(1, int(counts.max()))
    out = []
    for a in arrays:
        pad = np.zeros((ts,) + a.shape[1:], dtype=a.dtype); pad[:n_loc] = a
        every = np.frombuffer(comm.control.allgather(pad.tobytes()), dtype=a.dtype).reshape((comm.world, ts) + a.shape[1:])
        out.append(np.concatenate([every[r, :counts[r]] for r in range(comm.world)], axis=0))
    return out


def gather_ragged_dev(comm, part):
    """The device counterpart: ``part`` (this rank's DeviceOp, freed here as soon as it has been copied) goes into a shard of capacity
    ``ts = max(1, longest part)`` and :meth:`Communicator.allgather_op` gathers the shards.  Returns (the gathered operator of
    ``ts * world`` rows, the ranks' row counts, ts): rank r's rows are ``[r * ts, r * ts + counts[r])``.  The rows behind them are
    padding — identity rows with coefficient 0 — and must never reach a cleanup: they would be harmless for the sums but could take
    the identity's first-occurrence position.  What is done with the ranks' ranges is the caller's business."""
    n_loc, wq, _ = part.info()
    counts = np.frombuffer(comm.control.allgather(np.int64(n_loc).tobytes()), dtype=np.int64)
    ts = max(1, int(counts.max()))
    with kernels.DeviceOp.alloc(ts, wq, with_coeff=True) as shard:
        with part:
            shard.copy_rows_from(part, 0, n_loc)
        shard.set_rows(n_loc)
        full = kernels.DeviceOp.alloc(ts * comm.world, wq, with_coeff=True)
        try:
            comm.allgather_op(shard, full, ts * comm.world)
        except BaseException:
            full.free()
            raise
    return full, counts, ts


# ---- left-axis sharding of the all-pairs kernels ---------------------------------------------------------------------------------------
def sharded_commutes(a_rows_global, b_rows_local, n_b_total, comm, kernel=kernels.commutes):
    """This rank's block of ``commutes_termwise``: rows ``[begin, end)`` of the left operand against the WHOLE right
    operand (gathered from the per-rank shards).  ``kernel(a_block, b_full) -> bool[rows, M]`` defaults to the HIP
    commutation kernel; the CPU tests inject a checker to exercise the sharding/gather logic without a GPU."""
    _, bounds = shard_bounds(a_rows_global.shape[0], comm.world)
    b0, b1 = bounds[comm.rank]
    b_full = comm.allgather_rows_host(b_rows_local, n_b_total)
    return (b0, b1), kernel(np.ascontiguousarray(a_rows_global[b0:b1]), b_full)


def sharded_product(a_rows_global, a_coeff_global, b_rows_local, b_coeff_local, n_b_total, comm, kernel=kernels.mul_allpairs):
    """This rank's slab of the uncleaned product ``A * B`` with A (left factor) sharded along its term axis and B
    gathered: returns ((begin, end), rows, coeff) where row ``o*(end-begin) + i`` = ``A[begin+i] ^ B[o]``."""
    _, bounds = shard_bounds(a_rows_global.shape[0], comm.world)
    b0, b1 = bounds[comm.rank]
    b_full = comm.allgather_rows_host(b_rows_local, n_b_total)
    c = np.ascontiguousarray(b_coeff_local, dtype=np.complex128).view(np.float64).reshape(-1, 2)
    c_full = comm.allgather_rows_host(c.view('<u8'), n_b_total).view(np.float64).reshape(-1, 2).copy().view(np.complex128).reshape(-1)
    rows, coeff = kernel(np.ascontiguousarray(a_rows_global[b0:b1]), a_coeff_global[b0:b1], b_full, c_full, True)
    return (b0, b1), rows, coeff


# ---- product + cleanup, the outer index in contiguous blocks ----------------------------------------------------------------------------
def sharded_mul_cleanup(inner_rows, inner_coeff, outer_rows_local, outer_coeff_local, comm, inner_is_left=True, zero_threshold=1e-15,
                        mul_kernel=kernels.mul_cleanup, cleanup_kernel=kernels.cleanup):
    """Host arrays (CPU tests / the algorithm of :func:`sharded_mul_cleanup_dev`): this rank holds ALL of the inner operand and its
    contiguous block of the outer one (ranks in order).  ``mul_kernel(inner, ci, outer, co, inner_is_left, thr)`` = fused product +
    cleanup (thr None: keep everything), ``cleanup_kernel(rows, coeff, thr)`` = first-occurrence cleanup (the CPU tests inject their
    reference checker).  Returns the cleaned product (rows, coeff), identical on every rank."""
    rows, coeff = mul_kernel(inner_rows, inner_coeff, outer_rows_local, outer_coeff_local, inner_is_left, None)
    rows = np.ascontiguousarray(rows, dtype='<u8'); coeff = np.ascontiguousarray(coeff, dtype=np.complex128)
    if comm.world > 1:
        rows, coeff = gather_ragged(comm, rows, coeff)
    return cleanup_kernel(rows, coeff, zero_threshold)


def sharded_mul_cleanup_dev(comm, inner_full, outer_block, inner_is_left=True, zero_threshold=1e-15):
    """Fused product + cleanup of ``inner_full`` (all of one operand, on every rank — gather it with :meth:`Communicator.allgather_op`
    if it is sharded) with the OUTER operand sharded in contiguous blocks, ranks in order ("cleanup across GPUs").
    Pair ``(i, o)`` has index ``o * Ni + i`` in the reference (``_multiply_by_operator``, base.py:764-794): with the outer index
    sharded contiguously every pair of rank r precedes every pair of rank r + 1, so rank-major order IS the reference's order,
    and the first-occurrence order / sequential sums of ``symplectic_cleanup`` (utils.py:271-278) are those of
    (1) a local fused product + cleanup per rank WITHOUT threshold (a term may only cancel across ranks),
    (2) an all-gather of the cleaned partial operators (padded to the longest, then compacted in rank order),
    (3) one cleanup of the concatenation with the threshold — on every rank (the result is replicated).
    Sums associate per rank (exact for dyadic coefficients, <= 1e-16 relative otherwise), as in the tiled ``kernels.mul_cleanup``.
    Returns a DeviceOp."""
    part = kernels.mul_cleanup_handles(inner_full, outer_block, inner_is_left, None)
    if not comm.gathers:
        with part:
            return kernels.cleanup_dev(part, zero_threshold)
    full, counts, ts = gather_ragged_dev(comm, part)
    total = int(counts.sum())
    with full:
        # compact: rank r's rows one after the other, the padding left behind
        cat = kernels.DeviceOp.alloc(max(1, total), full.info()[1], with_coeff=True)
        pos = 0
        for r in range(comm.world):
            cat.copy_rows_from(full, r * ts, int(counts[r]), pos)
            pos += int(counts[r])
    with cat:
        cat.set_rows(total)
        return kernels.cleanup_dev(cat, zero_threshold)


# ---- cleanup across GPUs by HASH PARTITION ("cleanup across GPUs") -----------------------------------
# sharded_mul_cleanup above splits the OUTER index in contiguous blocks: every rank cleans its own slab, gathers every other rank's cleaned
# slab and cleans the concatenation again.  That is right for products whose duplicates sit close together, but the twins (i, o) / (o, i)
# of a squared operator live on different ranks, nothing merges locally, and every rank receives and re-cleans (nearly) the whole product.
#
# Here the PAIRS are partitioned by a GF(2)-LINEAR class of their product row: cls(row) = parities of the row under a few fixed random
# masks, so cls(inner[i] ^ outer[o]) = cls(inner[i]) ^ cls(outer[o]) — the owner of a pair, (cls_i ^ cls_o) mod G, is known from the two
# operand tables alone, equal product rows always have the same owner, and the pairs of one owner are a union of full sub-products
# (inner rows of class a) x (outer rows whose class XOR a maps to the owner).  No key is generated for a pair that another rank owns and
# NOTHING is exchanged before the result: every duplicate of a row meets its partners on its owner, which applies the threshold there.
# What does cross the wire is each rank's share of the FINAL result (rows, coefficients and the pair index of each row's first
# occurrence), all-gathered and put in the reference's first-occurrence order (utils.py:271) by that index.
# Precondition: both operands complete on every rank (the all-gather of the right operand that the product path performs anyway).
# Sums associate per sub-product (in pair order inside it, the sub-products' sums then in order of their first pair): bit-exact for
# dyadic coefficients, <= 1e-16 relative otherwise — the same statement as for the tiled kernels.mul_cleanup.
def linear_row_classes(rows, n_bits, seed=0x51A55E5):
    """GF(2)-linear class in [0, 2^n_bits) of every packed row: bit k = parity of the row under the k-th fixed random mask."""
    rows = np.ascontiguousarray(rows, dtype='<u8')
    rng = np.random.default_rng(seed)
    masks = rng.integers(0, 1 << 63, size=(n_bits, rows.shape[1]), dtype=np.uint64) ^ (rng.integers(0, 2, size=(n_bits, rows.shape[1]), dtype=np.uint64) << np.uint64(63))
    cls = np.zeros(rows.shape[0], dtype=np.int64)
    for k in range(n_bits):
        par = packing.popcount_rows(rows & masks[k][None, :]) & 1
        cls |= par << k
    return cls


def class_bits(world):
    """Number of class bits for ``world`` ranks: at least as many classes as ranks."""
    n_bits = 1
    while (1 << n_bits) < world:
        n_bits += 1
    if world & (world - 1):
        n_bits += 2                                                # a class count that is not a multiple of G: four times as many classes even the shares out
    return n_bits


def owned_subproducts(cls_i, cls_o, rank, world):
    """The sub-products ``rank`` owns, one per inner class a: (indices of the inner rows of class a, indices of the outer rows whose
    class XOR a maps to the rank), both ascending — local pair order = global pair order restricted.  Empty ones are skipped."""
    for a in range(1 << class_bits(world)):
        ia = np.flatnonzero(cls_i == a)
        oa = np.flatnonzero(((cls_o ^ a) % world) == rank)
        if ia.size and oa.size:
            yield ia, oa


def _record(stats, pairs_owned, n_inner, n_outer, world, share_bytes):
    if stats is not None:
        stats.update(pairs_owned=int(pairs_owned), pairs_total=int(n_inner) * int(n_outer), keys_exchanged=0,
                     bytes_sent=int(share_bytes) if world > 1 else 0)


def hash_partition_local(inner_rows, inner_coeff, outer_rows, outer_coeff, rank, world, inner_is_left=True, zero_threshold=1e-15,
                         mul_kernel=None, cleanup_kernel=None, stats=None):
    """Rank ``rank``'s share of the cleaned product: the terms whose product row's linear class maps to this rank — complete (every duplicate
    of such a row is among this rank's pairs), thresholded, in first-occurrence order, with the pair index ``o * Ni + i`` of each term's
    first occurrence.  No communication.  -> (rows, coeff, first_pair_index)."""
    mul_kernel = mul_kernel or (lambda a, ca, b, cb, left: kernels.mul_cleanup_indexed(a, ca, b, cb, left, None))
    cleanup_kernel = cleanup_kernel or kernels.cleanup_indexed
    inner_rows = np.ascontiguousarray(inner_rows, dtype='<u8'); outer_rows = np.ascontiguousarray(outer_rows, dtype='<u8')
    inner_coeff = np.ascontiguousarray(inner_coeff, dtype=np.complex128); outer_coeff = np.ascontiguousarray(outer_coeff, dtype=np.complex128)
    Ni, No, W = inner_rows.shape[0], outer_rows.shape[0], inner_rows.shape[1]
    n_bits = class_bits(world)
    cls_i = linear_row_classes(inner_rows, n_bits); cls_o = linear_row_classes(outer_rows, n_bits)
    parts_r, parts_c, parts_g = [], [], []
    pairs_owned = 0
    for ia, oa in owned_subproducts(cls_i, cls_o, rank, world):
        pairs_owned += ia.size * oa.size
        r, c, i_f, o_f = mul_kernel(inner_rows[ia], inner_coeff[ia], outer_rows[oa], outer_coeff[oa], inner_is_left)
        parts_r.append(r); parts_c.append(c)
        parts_g.append(oa[np.asarray(o_f, dtype=np.int64)] * Ni + ia[np.asarray(i_f, dtype=np.int64)])   # pair index of the first occurrence (base.py:783-792)
    if parts_r:
        rows = np.concatenate(parts_r, axis=0); coeff = np.concatenate(parts_c); g = np.concatenate(parts_g)
        order = np.argsort(g, kind='stable')
        rows, coeff, g = np.ascontiguousarray(rows[order]), coeff[order], g[order]
        rows, coeff, first = cleanup_kernel(rows, coeff, zero_threshold)                   # duplicates across this rank's sub-products; the threshold: final
        g = g[np.asarray(first, dtype=np.int64)]
    else:
        rows, coeff, g = np.zeros((0, W), dtype='<u8'), np.zeros(0, dtype=np.complex128), np.zeros(0, dtype=np.int64)
    _record(stats, pairs_owned, Ni, No, world, rows.nbytes + coeff.nbytes + g.nbytes)
    return np.ascontiguousarray(rows, dtype='<u8'), np.ascontiguousarray(coeff), g


def hash_partition_local_dev(inner, outer, rank, world, inner_is_left=True, zero_threshold=1e-15, stats=None, classes=None, max_pairs=None):
    """:func:`hash_partition_local` with the operands and every intermediate on the DEVICE (``csrc/partition.hip``): ``inner`` / ``outer`` are
    complete DeviceOps; sub-operands are gathered on the device, each sub-product is one indexed fused product + cleanup, the parts are ordered
    by pair index and merged there.  Only the operands' rows visit the host once, for their class bits (``classes`` = (cls_i, cls_o) skips
    that).  Returns a DeviceOp that carries the pair index of every term's first occurrence (``kernels.op_first_index``).
    One indexed product call handles fewer than 2^32 pairs (``symgpu_mul_cleanup_indexed_dev``): a sub-product beyond ``max_pairs`` is cut
    along its OUTER index into pieces below it — the pieces are further parts of the same merge, which orders everything by pair index."""
    max_pairs = int(max_pairs) if max_pairs else (1 << 31)
    Ni, wq, _ = inner.info()
    No = outer.info()[0]
    if classes is None:
        n_bits = class_bits(world)
        cls_i = linear_row_classes(inner.download(with_coeff=False), n_bits)
        cls_o = cls_i if outer is inner else linear_row_classes(outer.download(with_coeff=False), n_bits)
    else:
        cls_i, cls_o = classes
    parts, pairs_owned = [], 0
    try:
        for ia, oa in owned_subproducts(cls_i, cls_o, rank, world):
            pairs_owned += ia.size * oa.size
            step = max(1, max_pairs // int(ia.size))                                       # outer rows per call: ia.size * step <= max_pairs < 2^32
            with kernels.op_gather(inner, ia) as sub_i:
                for o0 in range(0, int(oa.size), step):
                    oc = oa[o0:o0 + step]
                    with kernels.op_gather(outer, oc) as sub_o:
                        parts.append(kernels.mul_cleanup_indexed_dev(sub_i, sub_o, inner_is_left, None))
                    kernels.part_global_index(parts[-1], ia, oc, Ni)
        if parts:
            res = kernels.merge_indexed_dev(parts, max(1, int(Ni * No - 1).bit_length()), True, zero_threshold)
        else:
            res = kernels.DeviceOp.alloc(1, wq, with_coeff=True)
            kernels.op_set_first_index(res, np.zeros(0, dtype='<u8'))
    finally:
        for p in parts:
            p.free()
    _record(stats, pairs_owned, Ni, No, world, res.n_terms * (16 * wq + 16 + 8))
    return res


def hash_partitioned_mul_cleanup(inner_rows, inner_coeff, outer_rows, outer_coeff, comm, inner_is_left=True, zero_threshold=1e-15,
                                 mul_kernel=None, cleanup_kernel=None, stats=None):
    """``inner * outer`` (or ``outer * inner``) + cleanup with the PAIRS partitioned over the ranks by the linear class of their product
    row.  Host arrays in, the cleaned product (rows, coeff) out, identical on every rank and equal to the single-process result.
    ``mul_kernel(inner, ci, outer, co, inner_is_left) -> (rows, coeff, i_first, o_first)`` = fused product + cleanup WITHOUT threshold plus the
    first pair of every output row (default ``kernels.mul_cleanup_indexed``); ``cleanup_kernel(rows, coeff, thr) -> (rows, coeff, first)``
    (default ``kernels.cleanup_indexed``).  The CPU tests inject their own checker kernels.  ``stats`` (dict, optional) receives
    ``pairs_owned``, ``pairs_total``, ``keys_exchanged`` (always 0) and ``bytes_sent`` of this rank."""
    rows, coeff, g = hash_partition_local(inner_rows, inner_coeff, outer_rows, outer_coeff, comm.rank, comm.world, inner_is_left, zero_threshold,
                                          mul_kernel, cleanup_kernel, stats)
    if comm.world == 1:
        return rows, coeff
    # the result: every rank's share, all-gathered and ordered by first pair index
    rows, coeff, g = gather_ragged(comm, rows, coeff, g)
    order = np.argsort(g, kind='stable')
    return np.ascontiguousarray(rows[order]), np.ascontiguousarray(coeff[order])


def hash_partitioned_mul_cleanup_dev(comm, inner_full, outer_full, inner_is_left=True, zero_threshold=1e-15, stats=None, gather=True):
    """Fused product + cleanup of two device operators that are COMPLETE on every rank (after :meth:`Communicator.allgather_op`), the pairs
    partitioned over the ranks by the GF(2)-linear class of their product row (:func:`hash_partition_local_dev`): all duplicates of a row meet
    on one rank — also the twins (i, o) / (o, i) of a squared operator, which the contiguous split of :func:`sharded_mul_cleanup_dev` leaves on
    different ranks — no key and no partial product crosses the wire.  The rank's share is computed, ordered and merged on the device.
    ``gather=False`` returns this rank's share (a DeviceOp carrying the pair index of each term's first occurrence: the result stays
    sharded); otherwise the shares are all-gathered (rows and coefficients through :func:`gather_ragged_dev`, the 8-byte indices over the
    control plane) and ordered by pair index on every rank: the replicated result in the reference's first-occurrence order."""
    share = hash_partition_local_dev(inner_full, outer_full, comm.rank, comm.world, inner_is_left, zero_threshold, stats)
    if not gather or not comm.gathers:
        return share
    first, = gather_ragged(comm, kernels.op_first_index(share))
    full, counts, ts = gather_ragged_dev(comm, share)
    ends = np.cumsum(counts)
    parts = []
    try:
        with full:
            # cut: rank r's rows as a part of their own with their first indices; the merge is by index, without cleanup
            for r in range(comm.world):
                n_r = int(counts[r])
                parts.append(kernels.DeviceOp.alloc(max(1, n_r), full.info()[1], with_coeff=True))
                parts[-1].copy_rows_from(full, r * ts, n_r)
                parts[-1].set_rows(n_r)
                kernels.op_set_first_index(parts[-1], first[ends[r] - n_r:ends[r]])
        key_bits = max(1, int(inner_full.n_terms * outer_full.n_terms - 1).bit_length())
        return kernels.merge_indexed_dev(parts, key_bits, False)
    finally:
        for p in parts:
            p.free()
