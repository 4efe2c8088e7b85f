"""Host-side mirror of the activation arena of a 'strict' executor plan (csrc/net.hip build(), mode 3): where the forward leaves the fp16
tensors the 16-bit backward reads, and where its fp32-grade tensors sit in the six scratch slots.  Used by the tests to read a forward's
arena; checked against udapose_net_act_bytes on the CPU (tests/test_strict_cpu.py)."""


def _a(v):
    return (v + 255) // 256 * 256


def strict_layout(layers, K, N, H, W):
    """{name: byte offset} of the fp16 tensors (x8, stem.y, stem.z, pool, poolidx, block{i}.{c1,c2,c3,cd}.y, block{i}.{b1,b2,b3,bd}.z,
    block{i}.mask, up{i}.y, up{i}.z, head_out) plus 'slot.<k>' for the scratch slots, with 'fslot.<tensor>' naming the slot of the
    forward's fp32-grade copy of a tensor, and 'act_bytes'."""
    slots = ["Y", "A", "B", "MID", "MID2", "DS"]

    def walk(sizes):
        need = {k: 0 for k in slots}
        off = {}
        cur = [sum(_a(sizes[k]) for k in slots) if sizes else 0]

        def alloc(name, nbytes):
            off[name] = cur[0]
            cur[0] = _a(cur[0] + nbytes)

        def take(name, slot, nbytes):
            need[slot] = max(need[slot], _a(nbytes))
            off["fslot." + name] = slot

        def conv(name, Ho, Wo, Co):
            alloc(name + ".y", N * Ho * Wo * Co * 2)
            take(name + ".y", "Y", N * Ho * Wo * Co * 4)

        def bn(name, C, npix, slot):
            alloc(name + ".save", 3 * C * 4)
            alloc(name + ".z", npix * C * 2)
            take(name + ".z", slot, npix * C * 4)

        alloc("x8", N * H * W * 8 * 2)
        take("x8", "DS", N * H * W * 8 * 4)
        Hs, Ws = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
        conv("stem", Hs, Ws, 64)
        bn("stem", 64, N * Hs * Ws, "B")
        Hp, Wp = (Hs + 2 - 3) // 2 + 1, (Ws + 2 - 3) // 2 + 1
        alloc("pool", N * Hp * Wp * 64 * 2)
        take("pool", "A", N * Hp * Wp * 64 * 4)
        alloc("poolidx", N * Hp * Wp * 64)
        cur_slot, Hc, Wc, Cc = "A", Hp, Wp, 64
        i = 0
        for L, nb in enumerate(layers):
            P = (64, 128, 256, 512)[L]
            for bi in range(nb):
                stride = 2 if (bi == 0 and L > 0) else 1
                out_slot = "B" if cur_slot == "A" else "A"
                pre = f"block{i}"
                conv(pre + ".c1", Hc, Wc, P)
                bn(pre + ".b1", P, N * Hc * Wc, "MID")
                Ho, Wo = (Hc + 2 - 3) // stride + 1, (Wc + 2 - 3) // stride + 1
                conv(pre + ".c2", Ho, Wo, P)
                bn(pre + ".b2", P, N * Ho * Wo, "MID2")
                conv(pre + ".c3", Ho, Wo, 4 * P)
                bn(pre + ".b3", 4 * P, N * Ho * Wo, out_slot)
                alloc(pre + ".mask", N * Ho * Wo * 4 * P // 8)
                if bi == 0:
                    conv(pre + ".cd", Ho, Wo, 4 * P)
                    bn(pre + ".bd", 4 * P, N * Ho * Wo, "DS")
                cur_slot, Hc, Wc, Cc = out_slot, Ho, Wo, 4 * P
                i += 1
        for u in range(3):
            Hc, Wc = Hc * 2, Wc * 2
            conv(f"up{u}", Hc, Wc, 256)
            cur_slot = "B" if cur_slot == "A" else "A"
            bn(f"up{u}", 256, N * Hc * Wc, cur_slot)
        alloc("head_out", N * Hc * Wc * K * 4)
        return need, off, cur[0]

    need, _, _ = walk(None)
    _, off, total = walk(need)
    o = 0
    for k in slots:
        off["slot." + k] = o
        o += _a(need[k])
    off["act_bytes"] = total
    return off
