"""Multi-GPU sharding of the all-pairs kernels — one process per GPU: the communicator.

The LEFT term axis is split into contiguous blocks, one per rank; every rank owns a 1/G shard of the packed RIGHT
operand, and ONE all-gather assembles the full right operand on every rank (RCCL ``ncclAllGather`` over xGMI through
``symgpu_comm_allgather_op``); each rank then computes its ``[N/G, M]`` block locally.  There is no reduction
collective anywhere on the path.  The reference has nothing comparable (its only parallelism is a CPU fork pool,
``symmer/process_handler.py``, off this path).  The algorithms on top of the communicator (sharded commutation, product and
product + cleanup) are functions of it in ``symmer_amd/sharding.py``.

Control plane (unique-id exchange, barriers, max-over-ranks timing; ``symmer_amd/control.py``): either a few lines of plain TCP
(``control='tcp'``, default of ``bench.py``: no PyTorch in the GPU processes at all) or ``torch.distributed`` with the gloo
backend (``control='gloo'``).  With ``data_plane='gloo-host'`` the all-gather itself runs over the control plane on host
arrays, which is what the CPU tests (world_size 2) exercise.

If RCCL cannot be brought up on EVERY rank (agreed over the control plane before anybody enters the collective
``ncclCommInitRank``), the communicator falls back to ``data_plane='host-staged'``: the same all-gather, but D2H ->
control plane -> H2D.  The step still exchanges the shards (3.2 MB per rank in the benchmark, a few ms next to a 0.45 s
step); callers report the degraded data plane (``Communicator.degraded``).  Nothing ever silently replicates data.
"""
import os
import sys
import ctypes
import numpy as np
from . import _lib, kernels
from .control import GlooControl, SoloControl, TcpControl


def shard_bounds(n_rows, world):
    """Contiguous equal blocks of ``ceil(n_rows/world)`` rows; tail ranks may be short or empty.
    Returns (Ts, [(begin, end)] per rank)."""
    ts = (n_rows + world - 1) // world if world > 0 else n_rows
    return ts, [(min(n_rows, r * ts), min(n_rows, (r + 1) * ts)) for r in range(world)]


class _stdout_to_stderr:
    """RCCL prints a version banner on file descriptor 1 when a communicator is created; callers such as bench.py promise ONE
    JSON line on stdout, so the C-level stdout is pointed at stderr while RCCL initialises.  The redirect is process wide, so it
    is only ever entered and left on the MAIN thread (never inside a watchdog thread that may not come back)."""

    def __enter__(self):
        sys.stdout.flush()
        self._saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        try:
            ctypes.CDLL(None).fflush(None)                          # the banner sits in the C stdio buffer: flush it while redirected
        except Exception:
            pass
        os.dup2(self._saved, 1)
        os.close(self._saved)
        return False


class CollectiveHang(RuntimeError):
    """A collective did not return on some rank within its time limit.  The stream it was enqueued on cannot be used again, so
    there is no data plane to fall back to in this process: every rank raises this after the ranks have agreed, and the caller
    (bench.py) reports it and ends the process with a non-zero status."""


def _run_with_watchdog(fn, timeout):
    """Run ``fn()`` on a daemon thread and wait at most ``timeout`` seconds for it, with file descriptor 1 pointed at stderr for
    the duration (on THIS thread, restored whatever happens to the worker).  Returns (status, error text, thread): status 0 =
    returned, 1 = raised, 2 = still running."""
    import threading
    result = {}

    def _body():
        try:
            fn()
            result['ok'] = True
        except Exception as exc:                               # noqa: BLE001 - reported through the caller's agreement
            result['error'] = str(exc) or type(exc).__name__

    th = threading.Thread(target=_body, daemon=True)
    with _stdout_to_stderr():
        th.start()
        th.join(timeout)
    if th.is_alive():
        return 2, 'did not return within the time limit', th
    if 'error' in result:
        return 1, result['error'], None
    return 0, None, None


class Communicator:
    def __init__(self, rank=0, world=1, data_plane='none', control=None):
        self.rank, self.world, self.data_plane = rank, world, data_plane
        self.control = control or SoloControl()
        self.rccl_error = None
        self.degraded = None      # text when the data plane is not the one asked for (host-staged instead of RCCL)
        self.gathers = False      # True when the right operand must be assembled with the all-gather
        self._hung_thread = None  # a watchdog thread that is still inside RCCL: the communicator must not be destroyed under it
        self._gather_checked = False   # the first all-gather runs under a watchdog and is agreed on by all ranks
        self.needs_hard_exit = False

    # ---- construction ------------------------------------------------------------------------------------
    @classmethod
    def from_env(cls, data_plane='rccl', control='tcp'):
        """RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT as set by ``torch.distributed.run``."""
        world = int(os.environ.get('WORLD_SIZE', '1'))
        rank = int(os.environ.get('RANK', '0'))
        # SYMGPU_FORCE_COMM=1 exercises the whole multi-rank path (control plane, RCCL init, all-gather) with ONE rank
        forced = os.environ.get('SYMGPU_FORCE_COMM', '0') == '1'
        if world == 1 and not forced:
            return cls(0, 1, 'none')
        addr = os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        mport = int(os.environ.setdefault('MASTER_PORT', '29531'))
        if control == 'gloo':
            plane = GlooControl(rank, world)
        else:
            # MASTER_PORT itself belongs to the launcher's store; use a derived port for our own socket
            port = int(os.environ.get('SYMGPU_CONTROL_PORT', 1024 + (mport + 7919) % 60000))
            plane = TcpControl(rank, world, addr, port)
        self = cls(rank, world, data_plane, plane)
        self.gathers = True
        if data_plane == 'rccl':
            self._init_rccl()
        return self

    def _fallback(self, why):
        """RCCL is unavailable: gather through host memory over the control plane instead (still a real exchange)."""
        self.rccl_error = why
        self.data_plane = 'host-staged'
        self.degraded = f'host-staged all-gather over the control plane (RCCL unavailable: {why})'

    def _agree(self, local_error, elsewhere_text):
        """The agreement that follows every step that can fail on one rank only: ``local_error`` is this rank's failure (None: the
        step went through here).  Returns None when it went through on every rank, otherwise the text all ranks act on — this
        rank's own error, or ``elsewhere_text`` on the ranks that have none."""
        if self.max_over_ranks(1.0 if local_error else 0.0) > 0.0:
            return local_error or elsewhere_text
        return None

    def _init_rccl(self):
        """RCCL communicator over the control plane.  Every step that can fail locally is followed by an agreement over the
        control plane, and the first agreement — "librccl loads on this rank" — happens BEFORE any rank enters the collective
        ``ncclCommInitRank``: a rank that failed locally would otherwise leave its peers blocked inside it.  Either ALL ranks
        end up with a communicator or all of them fall back to the host-staged data plane."""
        self.rccl_error = None
        local = None
        try:
            with _stdout_to_stderr():
                _lib.check(_lib.load().symgpu_comm_available())
        except Exception as exc:
            local = str(exc)
        why = self._agree(local, 'librccl could not be loaded on another rank')
        if why:
            return self._fallback(why)
        raw = (ctypes.c_uint8 * 128)()
        if self.rank == 0:
            try:
                with _stdout_to_stderr():
                    _lib.check(_lib.lib().symgpu_comm_unique_id(ctypes.addressof(raw)))
            except Exception as exc:                              # broadcast an all-zero id: everybody falls back
                local = str(exc)
                raw = (ctypes.c_uint8 * 128)()
        ident = self.control.bcast(bytes(raw), 128)
        if not any(ident):
            return self._fallback(local or 'rank 0 could not create an RCCL unique id')
        # ncclCommInitRank is collective and has no timeout of its own: run it on a watchdog thread, so that a bring-up that never
        # returns on some rank (fabric / IPC trouble) ends in the host-staged plane and a `degraded` line instead of a hung job
        raw = (ctypes.c_uint8 * 128)(*ident)
        status, err, th = _run_with_watchdog(lambda: _lib.check(_lib.lib().symgpu_comm_init(ctypes.addressof(raw), self.rank, self.world)),
                                             float(os.environ.get('SYMGPU_RCCL_INIT_TIMEOUT', '180')))
        if status == 2:
            # given up: should ncclCommInitRank come back later, the library destroys its communicator instead of installing it
            _lib.load().symgpu_comm_abandon()
            self._hung_thread = th
            local = 'ncclCommInitRank ' + err
        elif status == 1:
            local = err
        why = self._agree(local, 'RCCL initialisation failed on another rank')
        if why:
            if local is None:
                _lib.load().symgpu_comm_destroy()
            return self._fallback(why)

    # ---- control plane -----------------------------------------------------------------------------------
    def barrier(self):
        self.control.barrier()

    def max_over_ranks(self, x):
        return self.control.max(x)

    # ---- data plane ----------------------------------------------------------------------------------------
    def allgather_op(self, shard, full, n_rows_total):
        """Device-resident: gather every rank's shard (capacity Ts) into ``full`` and trim it to ``n_rows_total``."""
        if not self.gathers:
            raise ValueError('allgather_op without a communicator: use the shard directly')
        if self.data_plane == 'rccl':
            def gather():
                _lib.check(_lib.lib().symgpu_comm_allgather_op(shard.handle, full.handle))
            if self._gather_checked:
                gather()
            else:
                def first():
                    gather()
                    _lib.check(_lib.lib().symgpu_sync())            # the collective is asynchronous: a hang shows at the synchronisation
                self._first_gather(first)
        if self.data_plane != 'rccl':
            self._allgather_op_host(shard, full)
        full.set_rows(n_rows_total)

    def _first_gather(self, do_gather):
        """The first collective after the bring-up, under a watchdog, followed by the agreement of all ranks (the same pattern as the
        initialisation): every rank returned -> RCCL stays; no return within SYMGPU_RCCL_GATHER_TIMEOUT seconds on any rank ->
        :class:`CollectiveHang` on every rank; otherwise an error on any rank -> all ranks destroy their communicator and use the
        host-staged plane (the caller then gathers through it)."""
        status, err, th = _run_with_watchdog(do_gather, float(os.environ.get('SYMGPU_RCCL_GATHER_TIMEOUT', '120')))
        if status == 2:
            self._hung_thread = th
        hung = self._agree(err if status == 2 else None, 'did not return on another rank')
        self._gather_checked = True
        if hung:
            raise CollectiveHang('the first RCCL all-gather ' + hung)
        failed = self._agree(('the first RCCL all-gather failed: ' + err) if status == 1 else None,
                             'the first RCCL all-gather failed on another rank')
        if failed:
            _lib.load().symgpu_comm_destroy()
            self._fallback(failed)

    def _gather_through_host(self, shard):
        """The host-staged gather: shard (padded with identity rows to its capacity Ts) -> D2H -> control plane.  Returns the rows of
        all ranks, rank r's at ``[r * Ts, (r + 1) * Ts)``, and their coefficients — None for a rows-only operand (commutation
        needs no coefficients), which is decided here."""
        t, wq, ts = shard.info()
        try:
            r, c = shard.download()
        except _lib.SymgpuError:
            r, c = shard.download(with_coeff=False), None
        rows = np.zeros((ts, 2 * wq), dtype='<u8'); rows[:t] = r
        all_rows = np.frombuffer(self.control.allgather(rows.tobytes()), dtype='<u8').reshape(self.world * ts, 2 * wq)
        if c is None:
            return all_rows, None
        coeff = np.zeros(ts, dtype=np.complex128); coeff[:t] = c
        return all_rows, np.frombuffer(self.control.allgather(coeff.tobytes()), dtype=np.complex128)

    def _allgather_op_host(self, shard, full):
        """The same gather through host memory, H2D into ``full`` at the rows' global indices."""
        all_rows, all_coeff = self._gather_through_host(shard)
        full.write(0, all_rows, all_coeff, all_rows.shape[0])

    def verify_allgather(self, shard, full, n_rows_total):
        """Self-check of the RCCL data plane (call once, outside any timed region): gather the same shards a second time through
        host memory over the control plane and compare them with the device result of ``allgather_op`` — rows and coefficients,
        bit for bit, at their global positions.  If ANY rank sees a difference, all ranks leave RCCL for the host-staged plane
        (``degraded`` says why).  Returns True when the data plane in use after the call delivered the right operand."""
        if not self.gathers or self.data_plane != 'rccl':
            return True
        exp_rows, exp_c = self._gather_through_host(shard)
        exp_rows = exp_rows[:n_rows_total]
        if exp_c is None:
            ok = np.array_equal(full.download(with_coeff=False), exp_rows)
        else:
            fr, fc = full.download()
            ok = np.array_equal(fr, exp_rows) and np.array_equal(fc.view(np.float64), exp_c[:n_rows_total].view(np.float64))
        differs = 'the RCCL all-gather delivered rows that differ from the shards'
        why = self._agree(None if ok else differs, differs)
        if why:
            _lib.load().symgpu_comm_destroy()
            self._fallback(why)
            self.allgather_op(shard, full, n_rows_total)
            return False
        return True

    def allgather_rows_host(self, local_rows, n_rows_total):
        """Host arrays over the control plane (CPU tests / PCIe staging): returns the full ``uint64[n_rows_total, W]`` array."""
        local_rows = np.ascontiguousarray(local_rows, dtype='<u8')
        ts = max(1, shard_bounds(n_rows_total, self.world)[0])
        W = local_rows.shape[1]
        pad = np.zeros((ts, W), dtype='<u8')
        pad[:local_rows.shape[0]] = local_rows
        return np.frombuffer(self.control.allgather(pad.tobytes()), dtype='<u8').reshape(self.world * ts, W)[:n_rows_total].copy()

    def close(self):
        hung = self._hung_thread is not None and self._hung_thread.is_alive()
        if self.data_plane == 'rccl' and self.gathers and not hung:
            _lib.load().symgpu_comm_destroy()
        self.control.close()
        self.control = SoloControl()
        # a thread of this process still inside RCCL: tearing the runtime down under it at interpreter exit can crash or hang — the
        # caller should finish its output and then leave through hard_exit_if_hung()
        self.needs_hard_exit = hung

    HUNG_EXIT_STATUS = 4

    def hard_exit_if_hung(self, status=None):
        """Call after the last line of output: if a watchdog thread never came back from RCCL, end the process without running the
        finalisers (library shutdown under a thread that is inside RCCL is not safe).  The exit status is NON-ZERO (4) by default:
        a thread stuck inside RCCL means the run did not use the data plane it was asked to use (the JSON line says ``degraded``),
        and a launcher that only reads exit codes must see that."""
        if getattr(self, 'needs_hard_exit', False):
            sys.stdout.flush(); sys.stderr.flush()
            os._exit(self.HUNG_EXIT_STATUS if status is None else status)


def padded_random_shard(my_rows, ts, n_qubits, seed):
    """Synthetic right-operand shard with capacity ``ts`` (the all-gather pads the unused tail with zeros)."""
    op = kernels.DeviceOp.random(ts, n_qubits, 0.3, seed)
    op.set_rows(my_rows)
    return op
