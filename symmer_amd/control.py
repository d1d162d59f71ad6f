"""Control plane of the multi-rank communicator (``symmer_amd/parallel.py``): unique-id exchange, barriers, max-over-ranks
agreement and timing, byte all-gathers.  Three classes with the same five methods —

    bcast(payload, nbytes)   rank 0's ``nbytes`` bytes on every rank
    max(x)                   the largest float of all ranks
    allgather(payload)       equal-sized byte strings of all ranks, concatenated in rank order
    barrier()                returns once every rank has entered it
    close()                  waits for every rank, then releases the plane

:class:`TcpControl` is a few lines of plain TCP (default of ``bench.py``: no PyTorch in the GPU processes at all — PyTorch wheels
bundle their own HIP runtime and RCCL, which must not be mixed with the system ones this library links to), :class:`GlooControl`
is ``torch.distributed`` with the gloo backend, :class:`SoloControl` is a world of one rank.  A ``Communicator`` holds exactly
one of them and never asks which.
"""


class SoloControl:
    """World size 1 without sockets: every collective is the identity."""

    def bcast(self, payload, nbytes):
        return payload

    def max(self, x):
        return x

    def allgather(self, payload):
        return payload

    def barrier(self):
        pass

    def close(self):
        pass


class TcpControl:
    """Minimal rank-0-rooted control plane over TCP: broadcast of bytes, max-reduce of a float, barrier."""

    N_CANDIDATE_PORTS = 8

    def __init__(self, rank, world, addr, port, timeout=300.0):
        """``port`` is the first of N_CANDIDATE_PORTS candidates (stride 101): rank 0 listens on the first one it can bind, the
        other ranks probe the candidates until one answers the handshake (magic derived from port and world size), so a port
        that happens to be taken by an unrelated service on the node does not break the job."""
        import socket, struct, time
        self.rank, self.world, self._struct = rank, world, struct
        self.peers = []
        host = addr if addr not in ('localhost',) else '127.0.0.1'
        ports = [1024 + (port - 1024 + 101 * k) % 64000 for k in range(self.N_CANDIDATE_PORTS)]
        magic = struct.pack('<4sHH', b'SYMG', port & 0xFFFF, world & 0xFFFF)
        if rank == 0:
            srv = None
            for p in ports:
                try:
                    srv = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
                    srv.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
                    srv.bind((host, p))
                    break
                except OSError:
                    srv.close()
                    srv = None
            if srv is None:
                raise OSError(f'control plane: none of the ports {ports} could be bound on {host}')
            srv.listen(world + 8)
            srv.settimeout(timeout)
            conns = {}
            while len(conns) < world - 1:
                c, _ = srv.accept()
                try:
                    c.settimeout(10.0)
                    hello = self._recv(c, len(magic) + 4)
                    r = struct.unpack('<i', hello[len(magic):])[0]
                    if hello[:len(magic)] != magic or not (0 < r < world) or r in conns:
                        raise ConnectionError('not a peer of this job')
                    c.sendall(magic)
                    c.settimeout(timeout)
                    conns[r] = c
                except (OSError, ConnectionError):
                    c.close()
            self.peers = [conns[r] for r in sorted(conns)]
            srv.close()
        else:
            deadline = time.time() + timeout
            c = None
            while c is None:
                for p in ports:
                    try:
                        s = socket.create_connection((host, p), timeout=5.0)
                    except OSError:
                        continue
                    try:
                        s.settimeout(10.0)
                        s.sendall(magic + struct.pack('<i', rank))
                        if self._recv(s, len(magic)) == magic:
                            c = s
                            break
                        s.close()
                    except (OSError, ConnectionError):
                        s.close()
                if c is None:
                    if time.time() > deadline:
                        raise TimeoutError(f'control plane: rank 0 did not answer on any of {ports} at {host}')
                    time.sleep(0.2)
            c.settimeout(timeout)
            self.peers = [c]

    @staticmethod
    def _recv(c, n):
        buf = bytearray(n)
        view, got = memoryview(buf), 0
        while got < n:
            k = c.recv_into(view[got:], n - got)
            if k == 0:
                raise ConnectionError('control-plane peer closed the connection')
            got += k
        return bytes(buf)

    def bcast(self, payload, nbytes):
        if self.rank == 0:
            for c in self.peers:
                c.sendall(payload)
            return payload
        return self._recv(self.peers[0], nbytes)

    def max(self, x):
        s = self._struct
        if self.rank == 0:
            vals = [float(x)] + [s.unpack('<d', self._recv(c, 8))[0] for c in self.peers]
            m = max(vals)
            for c in self.peers:
                c.sendall(s.pack('<d', m))
            return m
        self.peers[0].sendall(s.pack('<d', float(x)))
        return s.unpack('<d', self._recv(self.peers[0], 8))[0]

    def allgather(self, payload):
        """Equal-sized byte strings from every rank, concatenated in rank order, on every rank (through rank 0)."""
        n = len(payload)
        if self.rank == 0:
            parts = [payload] + [self._recv(c, n) for c in self.peers]
            whole = b''.join(parts)
            for c in self.peers:
                c.sendall(whole)
            return whole
        self.peers[0].sendall(payload)
        return self._recv(self.peers[0], n * self.world)

    def barrier(self):
        self.max(0.0)

    def close(self):
        self.barrier()
        for c in self.peers:
            try:
                c.close()
            except OSError:
                pass
        self.peers = []


class GlooControl:
    """``torch.distributed`` with the gloo backend (the CPU tests; a launcher that has already initialised the process group)."""

    def __init__(self, rank, world):
        import torch
        import torch.distributed as dist
        if not dist.is_initialized():
            dist.init_process_group(backend='gloo', rank=rank, world_size=world)
        self.rank, self.world, self._torch, self._dist = rank, world, torch, dist

    def bcast(self, payload, nbytes):
        torch = self._torch
        t = torch.tensor(list(payload), dtype=torch.uint8) if self.rank == 0 else torch.zeros(nbytes, dtype=torch.uint8)
        self._dist.broadcast(t, src=0)
        return bytes(t.tolist())

    def max(self, x):
        t = self._torch.tensor([float(x)], dtype=self._torch.float64)
        self._dist.all_reduce(t, op=self._dist.ReduceOp.MAX)
        return float(t[0])

    def allgather(self, payload):
        torch = self._torch
        mine = torch.frombuffer(bytearray(payload), dtype=torch.uint8)
        parts = [torch.zeros_like(mine) for _ in range(self.world)]
        self._dist.all_gather(parts, mine)
        return b''.join(bytes(p.numpy().tobytes()) for p in parts)

    def barrier(self):
        self._dist.barrier()

    def close(self):
        if self._dist.is_initialized():
            self._dist.barrier()
            self._dist.destroy_process_group()
