// hprt device side — the body of a shadow-grid kernel, included textually into k_shadow_grid (shadow_grid.hip) and k_distant_grid
// (distant_grid.hip).  No include guard: it is program text of the kernel it stands in, not a header of declarations.
//
// Persistent waves with the walks' chunked dequeue and entry window.  A lane is a small state machine — ray wanted, block
// wanted, the block's second triangle wanted, a record wanted, leaf box wanted (grid_lanes.h: SG_RAY .. SG_BOX) — and every
// iteration of the wave issues the loads of all its lanes' states together and waits once: a lane that starts a new ray costs the
// others no round trip of their own.  The lists are read from the grid's device image (../shadow_grid.h, ShadowGridImage): a
// 128-byte block per cell that holds the list's head and its first two candidates, vertices and all, and 48-byte records in list
// order for the rest, so that a ray's typical two or three candidates cost two or three 128-byte lines and as many dependent
// rounds.  DevScene::tris is not read.
//
// Textual, not a function template: the kernels have to come out of the compiler as they did when each held this loop itself, and
// a __forceinline__ template (lambda or functor insertions) changes the register allocation throughout (Kernel).
//
// The including kernel has the parameters (DevScene sc, <grid> g, queue, countPtr, countImm, RayStream rays, occ, workCounter,
// chunk, refillMin), where g has image, imageBytes, recordsAt, nNear and R, and defines two macros:
//
//   GRID_LANES_SETUP     statements before the loop: uniform values that GRID_LANES_RAY reads.  May read g; writes names of its own.
//   GRID_LANES_RAY       statements of the SG_RAY step, for the ray that has just arrived.  May read ro (origin), d (direction,
//                        origin to light), rayTMax, g and what GRID_LANES_SETUP defined; must write cell (the ray's cell, < the
//                        image's cell count), sub (its sixteenth of the cell, su | sv << 4) and lim (an entry is tested while its
//                        key <= lim).
//
// Both are undefined again at the end.

    const uint32_t n = countPtr ? *countPtr : countImm;
    const uint32_t lane = __lane_id();
    const auto boxRsrc = __builtin_amdgcn_make_buffer_rsrc((void *)sc.leafBox, 0, (int)(sc.nPrims * 32u), 0x00020000);
    const auto imgRsrc = __builtin_amdgcn_make_buffer_rsrc((void *)g.image, 0, (int)g.imageBytes, 0x00020000);      // (blocks, then records: one resource, 32-bit byte offsets)
    const float robust = 1 + 2 * gamma_n(3);
    GRID_LANES_SETUP
    int st = SG_IDLE;
    bool hit = false;
    uint32_t slot = 0u;
    // the list being read (the near list comes first, then the cell's): entry i of cnt is the one wanted or under test; recAt: the byte
    // offset of entry i's record (a cell's list: of entry 2's while i < 2); kwN: SG_BLOCK2, the key word of entry 2
    uint32_t i = 0u, cnt = 0u, recAt = 0u, kwN = 0u, cell = 0u;
    bool nearList = false;
    uint32_t ePrim = 0u;      // the candidate under test (entry i)
    uint32_t sub = 0u;        // the sixteenth of its cell the ray falls into
    vec3 ro, invDir;
    float rayTMax = 0.f, lim = 0.f;
    RayShear shear; shear.k0 = shear.k1 = false; shear.Sx = shear.Sy = shear.Sz = 0.f;
    bool moreWork = n > 0;
    uint32_t localNext = 0u, localEnd = 0u;
    uint32_t window = 0u, windowBase = 0xffffffffu;
    while (true) {
        // ---- idle lanes take the next rays of the queue (k_walk4's dequeue: chunks off the work counter, slots through the entry window) ----
        const unsigned long long idle = __ballot(st == SG_IDLE);
        if (moreWork && ((uint32_t)__popcll(idle) >= refillMin || idle == ~0ull)) {
            if (localNext >= localEnd) {
                uint32_t base = 0u;
                if (lane == 0) base = atomicAdd(workCounter, chunk);
                base = __builtin_amdgcn_readfirstlane(base);
                localNext = base < n ? base : n;
                localEnd = (base + chunk < n) ? base + chunk : n;
                if (localNext >= localEnd) moreWork = false;
                windowBase = 0xffffffffu;      // a new chunk: the window read ahead belongs to the old one
            }
            const uint32_t want = (uint32_t)__popcll(idle);
            const uint32_t base = localNext;
            localNext = (localNext + want < localEnd) ? localNext + want : localEnd;
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
            uint32_t slotW = 0u;
            if (queue) {
                if (windowBase != base) { window = (base + lane < localEnd) ? queue[base + lane] : 0u; windowBase = base; }
                slotW = __shfl(window, (int)rank);
                window = (localNext + lane < localEnd) ? queue[localNext + lane] : 0u;
                windowBase = localNext;
            }
            if (st == SG_IDLE) {
                const uint32_t idx = base + rank;
                if (idx < localEnd) { slot = queue ? slotW : idx; hit = false; st = SG_RAY; }
            }
        }
        if (__ballot(st != SG_IDLE) == 0ull) {
            if (!moreWork) break;
            continue;
        }
        // ---- the loads of every lane's state, issued together ----
        u32x4 r0 = {0u, 0u, 0u, 0u}, r1 = {0u, 0u, 0u, 0u}, r2 = {0u, 0u, 0u, 0u};
        u32x4 r3 = {0u, 0u, 0u, 0u};
        if (st == SG_RAY) {
            r0 = __builtin_bit_cast(u32x4, rays.a[slot]);
            r1 = __builtin_bit_cast(u32x4, rays.b[slot]);
        } else if (st == SG_BOX) {
            const uint32_t pi = ePrim & SG_PRIM_MASK;
            r0 = __builtin_amdgcn_raw_buffer_load_b128(boxRsrc, pi * 32u, 0, 0);
            r1 = __builtin_amdgcn_raw_buffer_load_b128(boxRsrc, pi * 32u + 16u, 0, 0);
        } else if (st != SG_IDLE) {
            // a triangle with the words in its fourth lanes always arrives in r0 - r2: the block's first, its second, a record's
            const uint32_t at = st == SG_BLOCK ? cell * 128u + 16u : st == SG_BLOCK2 ? cell * 128u + 64u : recAt;
            r0 = __builtin_amdgcn_raw_buffer_load_b128(imgRsrc, at, 0, 0);
            r1 = __builtin_amdgcn_raw_buffer_load_b128(imgRsrc, at + 16u, 0, 0);
            r2 = __builtin_amdgcn_raw_buffer_load_b128(imgRsrc, at + 32u, 0, 0);
            if (st == SG_BLOCK) r3 = __builtin_amdgcn_raw_buffer_load_b128(imgRsrc, cell * 128u, 0, 0);
        }
        asm volatile("" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3));
        // ---- one step of every lane ----
        // the leaf's own box, exactly, as k_walk4's leaf_reached evaluates it
        auto leaf_reached = [&](float lx, float ly, float lz, float hx, float hy, float hz) -> bool {
            float tEn;
            return slab_test(lx, hx, ly, hy, lz, hz, ro, invDir, invDir.x < 0, invDir.y < 0, invDir.z < 0, robust, &tEn) && tEn < rayTMax;
        };
        const int st0 = st;         // the state whose loads have arrived
        bool done = false;          // the ray's answer is known
        bool listEnd = false;       // the list being read holds nothing more for this ray
        bool doTest = false;        // r0 - r2 hold a candidate (ePrim) that the ray meets
        if (st0 == SG_RAY) {
            ro = vec3(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z));
            rayTMax = __uint_as_float(r0.w);
            const vec3 d(__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z));
            invDir = vec3(1 / d.x, 1 / d.y, 1 / d.z);
            shear = ray_shear(d, invDir);
            GRID_LANES_RAY
            i = 0u;
            if (g.nNear != 0u) { nearList = true; cnt = g.nNear; recAt = g.recordsAt; st = SG_OVER; }
            else { nearList = false; st = SG_BLOCK; }
        } else if (st0 == SG_BLOCK) {
            // r3: the block's head {count, record of entry 2, prim[0], key[0]}.  (i == 1: back after a leaf box that failed entry 0's hit)
            cnt = r3.x; recAt = g.recordsAt + r3.y * 48u;
            if (i == 0u) {
                if (cnt == 0u || sg_key(r3.w) > lim) listEnd = true;
                else if (sg_reaches(r3.w, sub)) { doTest = true; ePrim = r3.z; }
            }
        } else if (st0 == SG_BLOCK2) {
            doTest = true;
        } else if (st0 == SG_OVER) {
            // a key beyond the ray's limit ends a cell's list (near-list keys are 0); an entry whose triangle does not reach the
            // ray's sixteenth of the cell is passed over
            if (sg_key(r1.w) > lim) listEnd = true;
            else if (sg_reaches(r1.w, sub)) { doTest = true; ePrim = r0.w; }
        } else if (st0 == SG_BOX) {
            if (leaf_reached(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z), __uint_as_float(r0.w), __uint_as_float(r1.x), __uint_as_float(r1.y))) { hit = true; done = true; }
            else {
                // on with the entry behind the one under test: the block again for its second, else a record
                ++i;
                if (nearList || i > 2u) recAt += 48u;
                if (!nearList && i < 2u) st = SG_BLOCK;
                else if (i >= cnt) listEnd = true;
                else st = SG_OVER;
            }
        }
        bool boxWanted = false;
        if (doTest) {
            asm volatile("" : "+v"(r0), "+v"(r1), "+v"(r2));
            const vec3 p0(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z)), p1(__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z)),
                       p2(__uint_as_float(r2.x), __uint_as_float(r2.y), __uint_as_float(r2.z));
            float b0, b1, b2, t;
            if (tri_test(p0, p1, p2, ro, rayTMax, shear, &b0, &b1, &b2, &t)) {
                // a hit counts if the reference's walk reaches this primitive's leaf
                if (ePrim & SG_SINGLE) {
                    if (leaf_reached(fminf(fminf(p0.x, p1.x), p2.x), fminf(fminf(p0.y, p1.y), p2.y), fminf(fminf(p0.z, p1.z), p2.z),
                                     fmaxf(fmaxf(p0.x, p1.x), p2.x), fmaxf(fmaxf(p0.y, p1.y), p2.y), fmaxf(fmaxf(p0.z, p1.z), p2.z))) { hit = true; done = true; }
                } else boxWanted = true;
            }
        }
        if (boxWanted) st = SG_BOX;
        else if (!done && !listEnd) {
            // entry i is done with: whether the next one concerns the ray is known from the words that came with this one
            if (st0 == SG_BLOCK) {
                i = 1u;
                if (cnt <= 1u || sg_key(r1.w) > lim) listEnd = true;
                else if (sg_reaches(r1.w, sub)) { st = SG_BLOCK2; ePrim = r0.w; kwN = r2.w; }
                else { i = 2u; if (cnt <= 2u || sg_key(r2.w) > lim) listEnd = true; else st = SG_OVER; }
            } else if (st0 == SG_BLOCK2) {
                i = 2u;
                if (cnt <= 2u || sg_key(kwN) > lim) listEnd = true; else st = SG_OVER;
            } else if (st0 == SG_OVER) {
                ++i; recAt += 48u;
                if (i >= cnt || sg_key(r2.w) > lim) listEnd = true;
            }
        }
        if (listEnd) {
            if (nearList) { nearList = false; i = 0u; st = SG_BLOCK; }      // the near list is through: the cell's
            else done = true;
        }
        if (done) { occ[slot] = hit ? 1 : 0; st = SG_IDLE; }
    }
#undef GRID_LANES_SETUP
#undef GRID_LANES_RAY
