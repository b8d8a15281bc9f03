// tic_adaptive.cpp - host half of the per-image Huffman tables: the tree of the reference's HuffmanTree (huffman.py:137-194) built
// from symbol statistics, the table serialization of write_huffman_table (codec.py:73-84), and a strict decoder of such streams.
//
// Byte-exactness is decided by the tree: leaves enter a queue.PriorityQueue (CPython heapq) in first-occurrence order and are
// compared by frequency alone, so equal frequencies are ordered by the heap's own mechanics.  Heap::push / Heap::pop below are
// heapq.heappush / heappop (_siftdown / _siftup of Lib/heapq.py) step for step.
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/tinyimgcodec_hip.h"
#include "tic_adaptive.h"
#include "tic_entropy.h"

namespace tic {
namespace {

struct Node {
    unsigned long long freq;
    int left, right; // children (-1: leaf)
    int sym;         // bin of a leaf
};

struct Heap {
    std::vector<Node> &nodes;
    std::vector<int> h;
    bool lt(int a, int b) const { return nodes[a].freq < nodes[b].freq; } // HuffmanTree.__Node.__lt__ (huffman.py:127-128)
    void siftdown(size_t startpos, size_t pos) {
        const int item = h[pos];
        while (pos > startpos) {
            const size_t parentpos = (pos - 1) >> 1;
            const int parent = h[parentpos];
            if (lt(item, parent)) {
                h[pos] = parent;
                pos = parentpos;
                continue;
            }
            break;
        }
        h[pos] = item;
    }
    void siftup(size_t pos) {
        const size_t endpos = h.size(), startpos = pos;
        const int item = h[pos];
        size_t childpos = 2 * pos + 1;
        while (childpos < endpos) {
            const size_t rightpos = childpos + 1;
            if (rightpos < endpos && !lt(h[childpos], h[rightpos])) childpos = rightpos;
            h[pos] = h[childpos];
            pos = childpos;
            childpos = 2 * pos + 1;
        }
        h[pos] = item;
        siftdown(startpos, pos);
    }
    void push(int x) {
        h.push_back(x);
        siftdown(0, h.size() - 1);
    }
    int pop() {
        const int last = h.back();
        h.pop_back();
        if (h.empty()) return last;
        const int ret = h[0];
        h[0] = last;
        siftup(0);
        return ret;
    }
};

struct BitOut {
    uint8_t *p;
    size_t cap_bits, n = 0;
    bool overflow = false;
    void put(unsigned long long v, int bits) { // MSB first
        for (int i = bits - 1; i >= 0; i--) {
            if (n >= cap_bits) {
                overflow = true;
                return;
            }
            const uint8_t mask = (uint8_t)(0x80u >> (n & 7));
            if ((v >> i) & 1ull)
                p[n >> 3] |= mask;
            else
                p[n >> 3] &= (uint8_t)~mask;
            n++;
        }
    }
};

// One tree (HuffmanTree.__init__ + __create_huffman_table): codes of the bins [0, nbins) that occur; `order` receives the leaves in
// depth-first order, left (0) first - the insertion order of the reference's bidict.  False when a code exceeds max_len(bin).
template <typename MaxLen>
bool build_tree(const unsigned long long *count, const unsigned long long *first, int nbins, unsigned long long *code, uint8_t *len,
                std::vector<int> &order, MaxLen max_len) {
    std::vector<int> leaves;
    for (int b = 0; b < nbins; b++) {
        code[b] = 0;
        len[b] = 0;
        if (count[b]) leaves.push_back(b);
    }
    // __calc_freq's dict: first-occurrence order
    std::stable_sort(leaves.begin(), leaves.end(), [&](int a, int b) { return first[a] < first[b]; });
    std::vector<Node> nodes;
    nodes.reserve(2 * leaves.size());
    Heap q{nodes, {}};
    for (int b : leaves) {
        nodes.push_back({count[b], -1, -1, b});
        q.push((int)nodes.size() - 1);
    }
    while (q.h.size() >= 2) {
        const int u = q.pop(), v = q.pop();
        nodes.push_back({nodes[u].freq + nodes[v].freq, u, v, -1});
        q.push((int)nodes.size() - 1);
    }
    const int root = q.pop();
    struct Item { int node, depth; unsigned long long code; };
    std::vector<Item> stack{{root, 0, 0ull}};
    order.clear();
    bool ok = true;
    while (!stack.empty()) {
        const Item it = stack.back();
        stack.pop_back();
        const Node &nd = nodes[it.node];
        if (nd.left < 0) {
            if (it.depth > max_len(nd.sym)) ok = false;
            code[nd.sym] = it.code;
            len[nd.sym] = (uint8_t)std::min(it.depth, 255);
            order.push_back(nd.sym);
            continue;
        }
        const unsigned long long c = it.depth < 64 ? it.code << 1 : 0ull;
        stack.push_back({nd.right, it.depth + 1, c | 1ull}); // right after left
        stack.push_back({nd.left, it.depth + 1, c});
    }
    return ok;
}

struct BitIn {
    const uint8_t *p;
    size_t nbits, pos = 0;
    bool get(int n, unsigned long long &v) { // n <= 64
        if (n < 0 || pos + (size_t)n > nbits) return false;
        v = 0;
        for (int i = 0; i < n; i++, pos++) v = (v << 1) | ((p[pos >> 3] >> (7 - (pos & 7))) & 1u);
        return true;
    }
};

// Prefix-code decoder: a binary trie of the table's codewords.
struct Trie {
    struct T { int child[2] = {-1, -1}; int sym = -1; };
    std::vector<T> t{T{}};
    bool add(unsigned long long code, int n, int sym) {
        int at = 0;
        for (int i = n - 1; i >= 0; i--) {
            if (t[at].sym >= 0) return false; // a code runs through another's leaf
            const int b = (int)((code >> i) & 1ull);
            if (t[at].child[b] < 0) {
                t[at].child[b] = (int)t.size();
                t.push_back(T{});
            }
            at = t[at].child[b];
        }
        if (t[at].sym >= 0 || t[at].child[0] >= 0 || t[at].child[1] >= 0) return false; // duplicate, or a prefix of another
        t[at].sym = sym;
        return true;
    }
    bool read(BitIn &r, int &sym) const {
        int at = 0;
        while (t[at].sym < 0) {
            unsigned long long b;
            if (!r.get(1, b)) return false;
            at = t[at].child[b];
            if (at < 0) return false; // a path without a codeword
        }
        sym = t[at].sym;
        return true;
    }
};

// BitBuffer.read_int (bitbuffer.py:56-66): one's complement for negatives
inline int read_value(unsigned long long bits, int size) {
    if (size == 0) return 0;
    if ((bits >> (size - 1)) & 1ull) return (int)bits;
    return -(int)((~bits) & ((1ull << size) - 1ull));
}

} // namespace

int huffman_table_build(const unsigned long long *dc_count, const unsigned long long *dc_first, const unsigned long long *ac_count,
                        const unsigned long long *ac_first, unsigned long long *dc_code, uint8_t *dc_len, unsigned long long *ac_code,
                        uint8_t *ac_len, uint8_t *table, size_t table_cap, size_t *table_bits) {
    if (!dc_count || !dc_first || !ac_count || !ac_first || !dc_code || !dc_len || !ac_code || !ac_len || !table_bits) return TIC_E_ARG;
    if (!table && table_cap) return TIC_E_ARG;
    if (std::none_of(dc_count, dc_count + 16, [](unsigned long long c) { return c != 0; }) ||
        std::none_of(ac_count, ac_count + 256, [](unsigned long long c) { return c != 0; }))
        return TIC_E_ARG; // no symbol: the reference's calc_huffman_table raises IndexError
    std::vector<int> dc_order, ac_order;
    // code + value bits of one symbol fit kAdaptMaxSymbolBits; a DC code also fits write_huffman_table's 4-bit length (always: at
    // most 16 leaves), an AC code its 8 bits
    const bool dc_ok = build_tree(dc_count, dc_first, 16, dc_code, dc_len, dc_order,
                                  [](int c) { return std::min(15, kAdaptMaxSymbolBits - c); });
    const bool ac_ok = build_tree(ac_count, ac_first, 256, ac_code, ac_len, ac_order,
                                  [](int rs) { return kAdaptMaxSymbolBits - (rs & 15); });
    if (!dc_ok || !ac_ok) return TIC_E_RANGE;
    BitOut o{table, table_cap * 8};
    o.put(dc_order.size(), 16); // codec.py:74-78
    for (int c : dc_order) {
        o.put((unsigned)c, 4);
        o.put(dc_len[c], 4);
        o.put(dc_code[c], dc_len[c]);
    }
    o.put(ac_order.size(), 16); // codec.py:79-84
    for (int rs : ac_order) {
        o.put((unsigned)(rs >> 4), 4);
        o.put((unsigned)(rs & 15), 4);
        o.put(ac_len[rs], 8);
        o.put(ac_code[rs], ac_len[rs]);
    }
    if (o.overflow) return TIC_E_SPACE;
    if (o.n & 7) o.p[o.n >> 3] &= (uint8_t)(0xff00u >> (o.n & 7)); // zero padding of the last byte
    *table_bits = o.n;
    return TIC_OK;
}

unsigned long long adaptive_stream_bits(const unsigned long long *dc_count, const unsigned long long *ac_count, const uint8_t *dc_len,
                                        const uint8_t *ac_len, size_t table_bits) {
    unsigned long long bits = 128ull + table_bits;
    for (int rs = 0; rs < 256; rs++) bits += ac_count[rs] * (unsigned long long)(ac_len[rs] + (unsigned)(rs & 15));
    for (int c = 0; c < 16; c++) bits += dc_count[c] * (unsigned long long)(dc_len[c] + (unsigned)c);
    return bits;
}

int adaptive_stream_size(const unsigned long long *dc_count, const unsigned long long *dc_first, const unsigned long long *ac_count,
                         const unsigned long long *ac_first, size_t *bytes) {
    if (!bytes) return TIC_E_ARG;
    unsigned long long dc_code[16], ac_code[256];
    uint8_t dc_len[16], ac_len[256], table[kAdaptMaxTableBytes];
    size_t tbits = 0;
    const int rc = huffman_table_build(dc_count, dc_first, ac_count, ac_first, dc_code, dc_len, ac_code, ac_len, table, sizeof table, &tbits);
    if (rc) return rc;
    *bytes = (size_t)((adaptive_stream_bits(dc_count, ac_count, dc_len, ac_len, tbits) + 7) / 8);
    return TIC_OK;
}

void adaptive_host_stats(const int16_t *zz, size_t n, AdaptStats *st) {
    for (int i = 0; i < kAdaptBins; i++) st->count[i] = 0ull, st->first[i] = ~0ull;
    st->err = 0u;
    auto bit_len = [](int v) {
        unsigned a = (unsigned)(v < 0 ? -v : v);
        int s = 0;
        for (; a; a >>= 1) s++;
        return s;
    };
    auto hit = [&](int bin, unsigned long long key) {
        st->count[bin]++;
        if (key < st->first[bin]) st->first[bin] = key;
    };
    int prev_dc = 0;
    for (size_t b = 0; b < n; b++) {
        const int16_t *c = zz + b * 64;
        const int dsz = bit_len((int)c[0] - prev_dc); // codec.py:34-35: the first block raw
        prev_dc = c[0];
        if (dsz > 15) st->err = 1u;
        hit(kAdaptDcBin + (dsz & 15), b);
        int last = 63;
        while (last > 0 && c[last] == 0) last--; // trailing zeros: no symbols (huffman.py:16-17)
        int run = 0;
        unsigned long long ord = 0;
        for (int k = 1; k <= last; k++) {
            if (c[k] == 0) {
                run++;
                continue;
            }
            for (; run >= 16; run -= 16) hit(0xF0, b * 64ull + ord++); // ZRL (huffman.py:24-28)
            const int sz = bit_len(c[k]);
            if (sz > 15) st->err = 1u;
            hit((run << 4) | (sz & 15), b * 64ull + ord++);
            run = 0;
        }
        hit(0, b * 64ull + ord); // EOB (huffman.py:33)
    }
}

int entropy_size_adaptive(const int16_t *zz, int h, int w, size_t *bytes) {
    if (!bytes || h < 0 || w < 0) return TIC_E_ARG;
    const size_t n = num_blocks(h, w);
    if (n == 0 || !zz) return TIC_E_ARG; // no blocks: no symbol to build a table from (the reference raises IndexError)
    AdaptStats st;
    adaptive_host_stats(zz, n, &st);
    if (st.err) return TIC_E_RANGE;
    return adaptive_stream_size(st.count + kAdaptDcBin, st.first + kAdaptDcBin, st.count, st.first, bytes);
}

// The header's flag and read_huffman_table (codec.py:87-99): the tries of the host decoder, the entries for the device decoder's
// tables (t may be null); r is left at the payload's first bit.
static int parse_table(const uint8_t *data, size_t len, BitIn &r, Trie &dc, Trie &ac, AdaptTable *t, const char **why) {
    if (!data || len < 16) {
        *why = "stream shorter than its 16-byte header";
        return TIC_E_STREAM;
    }
    if (!(data[12] & 0x80)) { // write_uint(1 << 31, 32): bit 31 most significant bit first (codec.py:111)
        *why = "the header carries no embedded Huffman table";
        return TIC_E_STREAM;
    }
    r = BitIn{data, len * 8, 128};
    unsigned long long cnt;
    if (!r.get(16, cnt) || cnt == 0 || cnt > 16) {
        *why = "DC table: entry count missing or outside 1..16";
        return TIC_E_STREAM;
    }
    for (unsigned long long i = 0; i < cnt; i++) {
        unsigned long long cat, n, code;
        if (!r.get(4, cat) || !r.get(4, n) || !r.get((int)n, code)) {
            *why = "DC table truncated";
            return TIC_E_STREAM;
        }
        if (!dc.add(code, (int)n, (int)cat) || cat + n > (unsigned long long)kAdaptMaxSymbolBits) {
            *why = "DC table is not a prefix code";
            return TIC_E_STREAM;
        }
        if (t) t->dc_sym[i] = (uint8_t)cat, t->dc_len[i] = (uint8_t)n, t->dc_code[i] = code;
    }
    if (t) t->ndc = (int)cnt;
    if (!r.get(16, cnt) || cnt == 0 || cnt > 256) {
        *why = "AC table: entry count missing or outside 1..256";
        return TIC_E_STREAM;
    }
    for (unsigned long long i = 0; i < cnt; i++) {
        unsigned long long rs, n, code;
        if (!r.get(8, rs) || !r.get(8, n) || n + (rs & 15) > (unsigned long long)kAdaptMaxSymbolBits || !r.get((int)n, code)) {
            *why = "AC table truncated or a code longer than 64 bits";
            return TIC_E_STREAM;
        }
        if (!ac.add(code, (int)n, (int)rs)) {
            *why = "AC table is not a prefix code";
            return TIC_E_STREAM;
        }
        if (t) t->ac_sym[i] = (uint8_t)rs, t->ac_len[i] = (uint8_t)n, t->ac_code[i] = code;
    }
    if (t) t->nac = (int)cnt, t->payload_bit = r.pos;
    return TIC_OK;
}

int adaptive_parse_table(const uint8_t *data, size_t len, AdaptTable *t, const char **why) {
    const char *dummy;
    if (!why) why = &dummy;
    *why = "";
    BitIn r{nullptr, 0};
    Trie dc, ac;
    return parse_table(data, len, r, dc, ac, t, why);
}

bool adaptive_dec_tab_buildable(const AdaptTable &t) {
    for (int i = 0; i < t.ndc; i++)
        if (t.dc_len[i] == 0) return false;
    for (int i = 0; i < t.nac; i++)
        if (t.ac_len[i] == 0) return false;
    return true;
}

bool adaptive_dec_tab_build(const AdaptTable &t, AdaptDecTab *out) {
    memset(out, 0, sizeof *out);
    for (int k = 0; k < 2; k++) {
        const int n = k ? t.nac : t.ndc;
        struct Long { unsigned long long code; uint16_t ls; };
        std::vector<Long> longs;
        for (int i = 0; i < n; i++) {
            const int len = k ? t.ac_len[i] : t.dc_len[i];
            const unsigned long long code = k ? t.ac_code[i] : t.dc_code[i];
            const uint16_t ls = (uint16_t)((len << 8) | (k ? t.ac_sym[i] : t.dc_sym[i]));
            if (len == 0) return false;
            if (len <= kAdaptDecK) {
                const unsigned first = (unsigned)(code << (kAdaptDecK - len));
                for (unsigned j = 0; j < (1u << (kAdaptDecK - len)); j++) out->prim[k][first + j] = ls;
            } else {
                longs.push_back({code << (64 - len), ls});
            }
        }
        std::sort(longs.begin(), longs.end(), [](const Long &a, const Long &b) { return a.code < b.code; });
        out->nlong[k] = (uint32_t)longs.size();
        for (size_t i = 0; i < longs.size(); i++) out->long_code[k][i] = longs[i].code, out->long_ls[k][i] = longs[i].ls;
    }
    return true;
}

int adaptive_decode(const uint8_t *data, size_t len, int h, int w, int16_t *zz, const char **why) {
    const char *dummy;
    if (!why) why = &dummy;
    *why = "";
    BitIn r{nullptr, 0};
    Trie dc, ac;
    unsigned long long v;
    const int rc = parse_table(data, len, r, dc, ac, nullptr, why);
    if (rc) return rc;
    const size_t nb = num_blocks(h, w);
    long long dc_run = 0;
    for (size_t b = 0; b < nb; b++) {
        int16_t *c = zz + b * 64;
        memset(c, 0, 128);
        int sym;
        if (!dc.read(r, sym) || !r.get(sym, v)) {
            *why = "stream truncated or a code without a symbol (DC)";
            return TIC_E_STREAM;
        }
        dc_run += read_value(v, sym); // np.cumsum (codec.py:53)
        if (dc_run < -32768 || dc_run > 32767) {
            *why = "DC outside int16";
            return TIC_E_STREAM;
        }
        c[0] = (int16_t)dc_run;
        int pos = 1; // decode_run_length (huffman.py:36-38): l zeros then k per symbol, EOB's trailing 0 dropped
        for (;;) {
            if (!ac.read(r, sym) || !r.get(sym & 15, v)) {
                *why = "stream truncated or a code without a symbol (AC)";
                return TIC_E_STREAM;
            }
            if (sym == 0) break; // EOB (huffman.py:92-94)
            pos += sym >> 4;
            if (pos > 63) {
                *why = "block of more than 63 AC coefficients";
                return TIC_E_STREAM;
            }
            c[pos++] = (int16_t)read_value(v, sym & 15);
        }
    }
    return TIC_OK;
}

} // namespace tic
