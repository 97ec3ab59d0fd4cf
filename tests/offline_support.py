"""What the tests of the offline phase's powers and cubes share: n parties in one process over an in-process tagged network, and
interpolation on Python ints.  Nothing here touches the device until _run_parties is called."""
import asyncio


class _TaggedNet:
    """get_send_recv(i)(tag) -> (send, recv) for party i; hook(sender, tag, dest, msg) -> the message that travels (tampering, recording)"""

    def __init__(self, n, hook=None):
        self.n, self.q, self.hook = n, [dict() for _ in range(n)], hook

    def _queue(self, party, tag):
        return self.q[party].setdefault(tag, asyncio.Queue())

    def get_send_recv(self, i):
        def factory(tag):
            def send(dest, msg):
                self._queue(dest, tag).put_nowait((i, self.hook(i, tag, dest, msg) if self.hook else msg))

            return send, self._queue(i, tag).get

        return factory


def _run_parties(p, n, t, body, hook=None, return_exceptions=False):
    """body(co, i) for every party i over one network -> the list of results; 20 s for all of it"""
    from honeybadgermpc_amd._capi import Context
    from honeybadgermpc_amd.open_coalescer import OpenCoalescer

    async def main():
        net = _TaggedNet(n, hook)
        work = asyncio.gather(*[body(OpenCoalescer(p, n, t, i, net.get_send_recv(i)), i) for i in range(n)], return_exceptions=return_exceptions)
        return await asyncio.wait_for(work, 20)

    results = asyncio.run(main())
    Context.get(p).torch.cuda.synchronize()
    return results


def _coefficients(ys, p):
    """the polynomial of degree < n through (1, ys[0]) .. (n, ys[n-1]) on Python ints -> n coefficients"""
    n = len(ys)
    out = [0] * n
    for i in range(n):
        num, den = [1], 1
        for j in range(n):
            if j != i:
                num = [(a - (j + 1) * b) % p for a, b in zip([0] + num, num + [0])]
                den = den * (i - j) % p
        scale = ys[i] * pow(den, -1, p) % p
        for e in range(n):
            out[e] = (out[e] + scale * num[e]) % p
    return out


def _check_sharings(p, n, t, per_party_t, per_party_2t=None):
    """every column of per_party_t ([party][index] ints) is a sharing of degree <= t, of per_party_2t of degree <= 2t with the same
    constant -> the constants"""
    secrets = []
    for idx in range(len(per_party_t[0])):
        ct = _coefficients([per_party_t[i][idx] for i in range(n)], p)
        assert not any(ct[t + 1:]), idx
        if per_party_2t is not None:
            c2 = _coefficients([per_party_2t[i][idx] for i in range(n)], p)
            assert not any(c2[2 * t + 1:]) and c2[0] == ct[0], idx
        secrets.append(ct[0])
    return secrets


def _deal(secret, degree, n, p, rnd):
    """shares at points 1 .. n of a random polynomial of the given degree with the given constant"""
    poly = [secret % p] + [rnd.randrange(p) for _ in range(degree)]
    return [sum(c * pow(x, e, p) for e, c in enumerate(poly)) % p for x in range(1, n + 1)]
