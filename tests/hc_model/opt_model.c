/*
 * tests/hc_model/opt_model.c -- CPU model of the price-based optimal LZ4 block
 * parse of lz4m_compress_opt_batch (python-lz4_amd/csrc/lz4m_opt.hip), as
 * DESIGN.md section 9.7 defines it.  The HIP kernels must produce these bytes.
 * Plain C99; it builds on the tables, the level table and the sequence writer
 * of hc_model.c, which it includes (so this file alone is the translation
 * unit, and the HC models and the decoder come with it).
 *
 * The parse, serially (n >= 13; shorter blocks are one literal run):
 *   tables    h(p) = (LE32(src + p) * 2654435761) >> (32 - 13); head[h] the
 *             newest inserted position with that hash, chain[p] the distance
 *             from p to the previous position with p's hash (0: none within
 *             65535 bytes) -- section 9.1's tables; attempts by the same level
 *             table (level < 1 -> 9, > 9 -> 9, 3 -> 4 ... 9 -> 256);
 *   matches   for every q <= n - 12, with every position below q inserted:
 *             walk the chain newest first for at most `attempts` candidates
 *             within 65535 bytes, each measured forwards only, up to lim =
 *             min(n - 5 - q, 65535) bytes; L[q] is the longest (>= 4), O[q]
 *             its distance, the first (nearest) among equals; the walk stops
 *             at a match of lim bytes.  Positions after n - 12 have none;
 *   prices    backwards from cost[n] = 1 (the last token), lit[n] = 0:
 *             cost[p] is the exact size of src[p..n) when a sequence starts at
 *             p, lit[p] that encoding's leading literal run.
 *             literal: l = lit[p + 1] + 1, cost[p + 1] + 1 + (l >= 15 and
 *             (l - 15) % 255 == 0);
 *             match: for ml = L[p] down to max(4, L[p] - 63): 3 +
 *             ext_bytes(ml - 4) + cost[p + ml]; the cheapest, the longest
 *             among equals; a match wins a tie with the literal (lit[p] = 0);
 *   emit      follow the choices from 0; the size is cost[0] (asserted);
 *   output    the block is written only if cost[0] <= cap; otherwise the
 *             result is 0 and dst is not touched.
 */
#include <assert.h>

#include "hc_model.c"   /* the tables, the level table, the sequence writer, the decoder */

#define OPT_LENGTHS 64   /* K: match lengths priced per position */

/* L[q], O[q] for every q < n (0: no match) */
static void opt_matches(hc_state* s, uint16_t* L, uint16_t* O) {
    const uint8_t* src = s->src;
    const int32_t n = s->n, mflimit = n - 12;
    int32_t pl = 0, po = 0;   /* L and O of q - 1 */
    memset(L, 0, (size_t)n * sizeof(uint16_t));
    memset(O, 0, (size_t)n * sizeof(uint16_t));
    for (int32_t q = 0; q <= mflimit; ++q) {
        const int32_t lim = n - 5 - q < 65535 ? n - 5 - q : 65535;
        int32_t best = 0, off = 0;
        uint32_t cur = s->head[hc_hash(src + q)];
        for (int left = s->attempts; left > 0 && cur != 0 && q - (int32_t)(cur - 1) <= HC_MAX_DIST; --left) {
            const int32_t c = (int32_t)(cur - 1);
            /* the match of q - 1 at the same distance, less its first byte, is known to hold here */
            int32_t fwd = q - c == po && pl > 1 ? pl - 1 : 0;
            if (best >= 4 && src[c + best] != src[q + best]) {
                fwd = 0;   /* cannot beat the best so far (best < lim here): not measured */
            } else {
                while (fwd + 8 <= lim && memcmp(src + c + fwd, src + q + fwd, 8) == 0) fwd += 8;
                while (fwd < lim && src[c + fwd] == src[q + fwd]) ++fwd;
            }
            if (fwd >= 4 && fwd > best) {
                best = fwd;
                off = q - c;
                if (best == lim) break;   /* nothing longer exists */
            }
            const uint32_t d = s->chain[c & 0xFFFF];
            cur = d ? cur - d : 0;
        }
        L[q] = (uint16_t)best;
        O[q] = (uint16_t)off;
        pl = best;
        po = off;
        hc_insert_to(s, q + 1);
    }
}

/* cost[0] of the model's parse, the choices in M (M[p]: the match length taken
 * at p, 0: a literal); L, O from opt_matches */
static int32_t opt_prices(int32_t n, const uint16_t* L, uint16_t* M, int32_t* cost) {
    int32_t lit = 0;
    cost[n] = 1;
    for (int32_t p = n - 1; p >= 0; --p) {
        const int32_t l = lit + 1;
        const int32_t lc = cost[p + 1] + 1 + (l >= 15 && (l - 15) % 255 == 0);
        int32_t mc = INT32_MAX, mlen = 0;
        if (L[p]) {
            const int32_t lo = L[p] - (OPT_LENGTHS - 1) > 4 ? L[p] - (OPT_LENGTHS - 1) : 4;
            for (int32_t ml = L[p]; ml >= lo; --ml) {
                const int32_t c = 3 + ext_bytes(ml - 4) + cost[p + ml];
                if (c < mc) {   /* the longest among equals */
                    mc = c;
                    mlen = ml;
                }
            }
        }
        if (mlen && mc <= lc) {
            cost[p] = mc;
            M[p] = (uint16_t)mlen;
            lit = 0;
        } else {
            cost[p] = lc;
            M[p] = 0;
            lit = l;
        }
    }
    return cost[0];
}

/* the block's size (its cost[0]), written to dst if `write`; 0 on a bad
 * argument or, writing, where it does not fit in cap */
static int opt_run(const uint8_t* src, int n, uint8_t* dst, int cap, int level, int write) {
    if (n < 0 || cap < 0 || n > HC_MAX_INPUT) return 0;
    int64_t op = 0;
    if (n < 13) {   /* a token and n < 15 literals */
        if (!write) return 1 + n;
        return hc_emit(src, n, 0, 0, dst, &op, cap) ? (int)op : 0;
    }
    hc_state s;
    const int tables = hc_open(&s, src, n, level);
    uint16_t* L = (uint16_t*)malloc((size_t)n * sizeof(uint16_t));
    uint16_t* O = (uint16_t*)malloc((size_t)n * sizeof(uint16_t));
    uint16_t* M = (uint16_t*)malloc((size_t)n * sizeof(uint16_t));
    int32_t* cost = (int32_t*)malloc(((size_t)n + 1) * sizeof(int32_t));
    int size = 0;
    if (tables && L && O && M && cost) {
        opt_matches(&s, L, O);
        size = opt_prices(n, L, M, cost);
        if (write && size > cap) size = 0;
        if (write && size) {
            int32_t anchor = 0, p = 0;
            int fits = 1;
            while (p < n && fits) {
                if (M[p]) {
                    fits = hc_emit(src + anchor, p - anchor, O[p], M[p], dst, &op, size);
                    p += M[p];
                    anchor = p;
                } else {
                    ++p;
                }
            }
            fits = fits && hc_emit(src + anchor, n - anchor, 0, 0, dst, &op, size);
            assert(fits && op == size);
            if (!fits || op != size) abort();
        }
    }
    hc_close(&s);
    free(L);
    free(O);
    free(M);
    free(cost);
    return size;
}

int opt_model_compress(const uint8_t* src, int n, uint8_t* dst, int cap, int level) {
    return opt_run(src, n, dst, cap, level, 1);
}

/* cost[0] of the price pass alone (what opt_model_compress's size must equal) */
int opt_model_cost(const uint8_t* src, int n, int level) { return opt_run(src, n, NULL, 0, level, 0); }
