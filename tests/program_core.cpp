// The filter-program compiler (duckdb-cubit_amd/csrc/cubit_program.hpp, HIP-free) run on the CPU, built
// with AddressSanitizer and UBSan by tests/test_program_core.py. Every emitted program is run by the
// small interpreters below, written from the encoding documented at EvalProgram (not the library's
// code), on one random 64-bit word per leaf (64 assignments at once), against the direct value of the
// tree it came from. The first failed check prints its place and ends the program with status 1.
//
//   program_core trees N    N random trees (fixed seeds) and the directed ones; prints the form counts
//   program_core algebra    mk_not / mk_bin folding against the truth tables
//   program_core parser     the postfix parser: valid programs and each malformation
//   program_core walk       filter_subtree_end over prefix arrays and their truncations; the node check
//   program_core range      CmpRange membership, intersection and clamp32 at the INT64 edges
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "cubit_program.hpp"

using namespace cubit;

#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                             \
            std::printf("\n");                                    \
            std::exit(1);                                         \
        }                                                         \
    } while (0)

namespace {

using Rng = std::mt19937_64;

// the words the leaves point at: leaf i reads words[i]
constexpr int kWords = 64;
uint64_t g_words[kWords];

// ---------------------------------------------------------------- the test's own tree and values

// What the generator means, evaluated without the library: the reference of every check.
struct Spec {
    enum Kind { LEAF, CONST, NOT, AND, OR, ANDNOT } kind = CONST;
    int id = 0;        // LEAF: its word
    bool flag = false; // LEAF: complemented; CONST: the value
    std::unique_ptr<Spec> a, b;
};
using SpecP = std::unique_ptr<Spec>;

uint64_t value_of(const Spec& s) {
    switch (s.kind) {
    case Spec::LEAF: return s.flag ? ~g_words[s.id] : g_words[s.id];
    case Spec::CONST: return s.flag ? ~0ull : 0ull;
    case Spec::NOT: return ~value_of(*s.a);
    case Spec::AND: return value_of(*s.a) & value_of(*s.b);
    case Spec::OR: return value_of(*s.a) | value_of(*s.b);
    default: return value_of(*s.a) & ~value_of(*s.b);
    }
}
ExprP build(const Spec& s) {
    switch (s.kind) {
    case Spec::LEAF: {
        Leaf l;
        l.bv = &g_words[s.id];
        return mk_leaf(l, s.flag);
    }
    case Spec::CONST: return s.flag ? mk_true() : mk_false();
    case Spec::NOT: return mk_not(build(*s.a));
    case Spec::AND: return mk_bin(Expr::AND, build(*s.a), build(*s.b));
    case Spec::OR: return mk_bin(Expr::OR, build(*s.a), build(*s.b));
    default: return mk_bin(Expr::ANDNOT, build(*s.a), build(*s.b));
    }
}
// the library's expression, evaluated node by node
uint64_t value_of(const ExprP& e) {
    switch (e->kind) {
    case Expr::LEAF: return e->neg ? ~*e->leaf.bv : *e->leaf.bv;
    case Expr::CONST_TRUE: return ~0ull;
    case Expr::CONST_FALSE: return 0ull;
    case Expr::AND: return value_of(e->a) & value_of(e->b);
    case Expr::OR: return value_of(e->a) | value_of(e->b);
    default: return value_of(e->a) & ~value_of(e->b);
    }
}
bool is_const(const ExprP& e) { return e->kind == Expr::CONST_TRUE || e->kind == Expr::CONST_FALSE; }
// no constant survives below the root, and only leaves are complemented
void check_folded(const ExprP& e, bool root = true) {
    if (is_const(e)) {
        CHECK(root, "a constant below the root");
        return;
    }
    if (e->kind == Expr::LEAF) return;
    CHECK(e->a && e->b, "a binary node without two children");
    check_folded(e->a, false);
    check_folded(e->b, false);
}
// a conjunction of literals: AND nodes, and a & ~leaf
bool is_literal_conjunction(const ExprP& e) {
    if (e->kind == Expr::LEAF) return true;
    if (e->kind == Expr::AND) return is_literal_conjunction(e->a) && is_literal_conjunction(e->b);
    if (e->kind == Expr::ANDNOT) return e->b->kind == Expr::LEAF && is_literal_conjunction(e->a);
    return false;
}

SpecP leaf_spec(int id, bool neg) {
    auto s = std::make_unique<Spec>();
    s->kind = Spec::LEAF;
    s->id = id;
    s->flag = neg;
    return s;
}
SpecP const_spec(bool v) {
    auto s = std::make_unique<Spec>();
    s->kind = Spec::CONST;
    s->flag = v;
    return s;
}
SpecP not_spec(SpecP a) {
    auto s = std::make_unique<Spec>();
    s->kind = Spec::NOT;
    s->a = std::move(a);
    return s;
}
SpecP bin_spec(Spec::Kind k, SpecP a, SpecP b) {
    auto s = std::make_unique<Spec>();
    s->kind = k;
    s->a = std::move(a);
    s->b = std::move(b);
    return s;
}

// ---------------------------------------------------------------- interpreters of EvalProgram

uint64_t literal(const EvalProgram& p, uint32_t k) {
    const uint64_t w = *p.leaf[k];
    return ((p.negate >> k) & 1u) ? ~w : w;
}

struct PostfixRun {
    uint64_t value = 0;
    int depth = 0;  // the deepest the stack got
    int ops = 0;
};
// leaf k pushed, complemented per negate, then nops(k) ops (2 bits each, in order, from `ops`)
PostfixRun run_postfix(const EvalProgram& p) {
    PostfixRun r;
    std::vector<uint64_t> st;
    for (uint32_t k = 0; k < p.n_leaves; ++k) {
        st.push_back(literal(p, k));
        r.depth = std::max(r.depth, (int)st.size());
        const uint32_t n = (p.nops >> (4 * k)) & 15u;
        for (uint32_t t = 0; t < n; ++t) {
            CHECK(st.size() >= 2, "postfix underflow at leaf %u", k);
            CHECK(r.ops < kMaxOps, "more than %d ops", kMaxOps);
            const uint32_t op = (p.ops >> (2 * r.ops++)) & 3u;
            const uint64_t b = st.back();
            st.pop_back();
            const uint64_t a = st.back();
            st.pop_back();
            CHECK(op == OP_AND || op == OP_OR || op == OP_ANDNOT, "opcode %u", op);
            st.push_back(op == OP_AND ? (a & b) : op == OP_OR ? (a | b) : (a & ~b));
        }
    }
    CHECK(st.size() == 1, "the postfix run ends with %zu values", st.size());
    r.value = st[0];
    return r;
}
uint64_t run_conj(const EvalProgram& p) {
    uint64_t r = ~0ull;
    for (uint32_t k = 0; k < p.n_leaves; ++k) r &= literal(p, k);
    return r;
}
// groups of literals (leaf 0 and every leaf with its gstart bit open one): DNF = OR of ANDs, CNF = AND of ORs
uint64_t run_two_level(const EvalProgram& p, bool dnf) {
    uint64_t r = dnf ? 0ull : ~0ull, cur = 0;
    for (uint32_t k = 0; k < p.n_leaves; ++k) {
        const uint64_t x = literal(p, k);
        if (k == 0) {
            cur = x;
        } else if ((p.gstart >> k) & 1u) {
            r = dnf ? (r | cur) : (r & cur);
            cur = x;
        } else {
            cur = dnf ? (cur & x) : (cur | x);
        }
    }
    return dnf ? (r | cur) : (r & cur);
}

// ---------------------------------------------------------------- one tree through the compiler

struct Tally {
    uint64_t trees = 0, constant = 0, accepted = 0, deep = 0, form[4] = {0, 0, 0, 0};
};

// every check the issue lists for a tree; returns the emitter for the directed cases
Emitter check_tree(const Spec& s, Tally& tally, const char* what) {
    const uint64_t want = value_of(s);
    const ExprP e = build(s);
    ++tally.trees;
    CHECK(value_of(e) == want, "%s: the built expression differs from the tree", what);
    check_folded(e);
    Emitter em;
    em.emit_top(e);
    if (is_const(e)) {
        ++tally.constant;
        CHECK(want == (e->kind == Expr::CONST_TRUE ? ~0ull : 0ull), "%s: folded to the wrong constant", what);
        CHECK(!em.ok && !fits(e), "%s: a constant was emitted", what);
        return em;
    }
    const int leaves = count_leaves(e);
    CHECK(em.ok == (leaves <= kMaxLeaves), "%s: ok %d with %d leaves", what, (int)em.ok, leaves);
    CHECK(fits(e) == (em.ok && em.max_depth <= 4), "%s: fits %d, ok %d, depth %d", what, (int)fits(e), (int)em.ok,
          em.max_depth);
    // refused or not, nothing was written past the arrays
    CHECK(em.prog.n_leaves <= (uint32_t)kMaxLeaves && em.n_ops <= kMaxOps, "%s: %u leaves, %d ops", what,
          em.prog.n_leaves, em.n_ops);
    if (!em.ok) return em;
    ++tally.accepted;
    const EvalProgram& p = em.prog;
    CHECK(p.n_leaves == (uint32_t)leaves, "%s: n_leaves %u, tree %d", what, p.n_leaves, leaves);
    uint32_t ops = 0;
    for (int k = 0; k < kMaxLeaves; ++k) {
        const uint32_t n = (p.nops >> (4 * k)) & 15u;
        CHECK(n <= 15u && ((uint32_t)k < p.n_leaves || n == 0), "%s: nibble %d = %u", what, k, n);
        ops += n;
    }
    CHECK(ops == p.n_leaves - 1 && ops <= (uint32_t)kMaxOps && (int)ops == em.n_ops, "%s: %u ops for %u leaves", what,
          ops, p.n_leaves);
    CHECK((p.negate >> p.n_leaves) == 0 && (p.gstart >> p.n_leaves) == 0, "%s: bits past the leaves", what);
    CHECK(p.form == FORM_POSTFIX || p.form == FORM_DNF || p.form == FORM_CNF, "%s: emitted form %u", what, p.form);
    const PostfixRun run = run_postfix(p);
    CHECK(run.value == want, "%s: the postfix program differs from the tree (form %u)", what, p.form);
    CHECK(run.ops == (int)ops, "%s: the run took %d ops of %u", what, run.ops, ops);
    const uint32_t form = eval_form(p);
    CHECK(form <= FORM_CNF, "%s: eval_form %u", what, form);
    ++tally.form[form];
    if (p.form == FORM_POSTFIX)  // emitted as postfix or conjunction
        CHECK(run.depth == em.max_depth, "%s: depth %d observed, max_depth %d", what, run.depth, em.max_depth);
    if (em.max_depth > 4) ++tally.deep;
    // CONJ exactly for a conjunction of literals. With two or more leaves that is the AND chain the
    // emitter writes; a single leaf is the chain of length one (no op), which is_conjunction takes too,
    // so it runs the K = 1 conjunction kernel
    const bool conj = is_literal_conjunction(e);
    CHECK((form == FORM_CONJ) == conj, "%s: eval_form %u, conjunction of literals %d", what, form, (int)conj);
    if (leaves == 1) CHECK(form == FORM_CONJ && p.form == FORM_POSTFIX && p.nops == 0, "%s: single leaf form %u", what, form);
    CHECK(is_conjunction(p) == (form == FORM_CONJ), "%s: is_conjunction disagrees with eval_form", what);
    const uint64_t by_form = form == FORM_CONJ ? run_conj(p)
                             : form == FORM_DNF ? run_two_level(p, true)
                             : form == FORM_CNF ? run_two_level(p, false)
                                                : run.value;
    CHECK(by_form == want, "%s: form %u differs from the tree", what, form);
    if (form == FORM_DNF || form == FORM_CNF) CHECK(p.gstart & 1u, "%s: leaf 0 opens no group", what);
    return em;
}

// ---------------------------------------------------------------- random trees

struct Gen {
    Rng rng;
    int next_id = 0;
    explicit Gen(uint64_t seed) : rng(seed) {}
    uint32_t below(uint32_t n) { return (uint32_t)(rng() % n); }
    bool chance(uint32_t percent) { return below(100) < percent; }
    SpecP literal(uint32_t neg_percent = 30) { return leaf_spec(next_id++, chance(neg_percent)); }
    // any shape over n leaves: the three ops, NOT above a subtree, a constant beside one
    SpecP any(int n) {
        SpecP s;
        if (n == 1) {
            s = literal();
        } else {
            const int l = 1 + (int)below((uint32_t)n - 1);
            const uint32_t o = below(10);
            s = bin_spec(o < 4 ? Spec::AND : o < 8 ? Spec::OR : Spec::ANDNOT, any(l), any(n - l));
        }
        if (chance(8)) s = not_spec(std::move(s));
        if (chance(4)) {
            const Spec::Kind k = (Spec::Kind)(Spec::AND + below(3));
            s = chance(50) ? bin_spec(k, std::move(s), const_spec(chance(50)))
                           : bin_spec(k, const_spec(chance(50)), std::move(s));
        }
        return s;
    }
    // n literals joined by `k` (AND: some as a & ~leaf), left- or right-leaning at random
    SpecP chain(int n, Spec::Kind k) {
        SpecP s = literal();
        for (int i = 1; i < n; ++i) {
            if (k == Spec::AND && chance(25)) s = bin_spec(Spec::ANDNOT, std::move(s), literal());
            else if (chance(70)) s = bin_spec(k, std::move(s), literal());
            else s = bin_spec(k, literal(), std::move(s));
        }
        return s;
    }
    // `groups` chains of `inner` joined by `outer`
    SpecP two_level(int groups, int max_group, Spec::Kind inner, Spec::Kind outer) {
        SpecP s = chain(1 + (int)below((uint32_t)max_group), inner);
        for (int g = 1; g < groups; ++g) s = bin_spec(outer, std::move(s), chain(1 + (int)below((uint32_t)max_group), inner));
        return s;
    }
    SpecP tree() {
        next_id = 0;
        const uint32_t style = below(100);
        // leaf counts: mostly within the 8 a program holds, a tail up to 20
        const int n = chance(70) ? 1 + (int)below(8) : 9 + (int)below(12);
        if (style < 55) return any(n);
        if (style < 65) return chain(std::min(n, 12), Spec::AND);
        if (style < 80) return two_level(2 + (int)below(3), 3, Spec::AND, Spec::OR);
        if (style < 95) return two_level(2 + (int)below(3), 3, Spec::OR, Spec::AND);
        return not_spec(two_level(2 + (int)below(2), 3, Spec::AND, Spec::OR));  // De Morgan: a CNF
    }
};

void fill_words(Rng& rng) {
    for (uint64_t& w : g_words) w = rng();
}

SpecP andnot_chain(int n) {  // l0 & ~(l1 & ~(l2 & ~ …))
    SpecP s = leaf_spec(n - 1, false);
    for (int i = n - 2; i >= 0; --i) s = bin_spec(Spec::ANDNOT, leaf_spec(i, false), std::move(s));
    return s;
}

void directed(Tally& tally) {
    Rng rng(7);
    fill_words(rng);
    {  // a right-deep ANDNOT chain of 8 leaves: accepted, 8 deep, not for the kernels' 4-deep stack
        const SpecP s = andnot_chain(8);
        const Emitter em = check_tree(*s, tally, "andnot chain 8");
        CHECK(em.ok && em.max_depth == 8 && !fits(build(*s)), "andnot chain 8: ok %d depth %d", (int)em.ok, em.max_depth);
        const SpecP s4 = andnot_chain(4);
        const Emitter em4 = check_tree(*s4, tally, "andnot chain 4");
        CHECK(em4.ok && em4.max_depth == 4 && fits(build(*s4)), "andnot chain 4: depth %d", em4.max_depth);
        const SpecP s5 = andnot_chain(5);
        CHECK(check_tree(*s5, tally, "andnot chain 5").max_depth == 5 && !fits(build(*s5)), "andnot chain 5");
    }
    {  // a & ~b, a a leaf: b a heavier subtree (order kept, ANDNOT), and b a leaf (a conjunction)
        const SpecP heavy = bin_spec(Spec::ANDNOT, leaf_spec(0, false),
                                     bin_spec(Spec::OR, bin_spec(Spec::AND, leaf_spec(1, false), leaf_spec(2, true)),
                                              bin_spec(Spec::AND, leaf_spec(3, false), leaf_spec(4, false))));
        const Emitter em = check_tree(*heavy, tally, "a & ~heavy");
        CHECK(em.ok && em.prog.leaf[0] == &g_words[0] && eval_form(em.prog) == FORM_POSTFIX, "a & ~heavy");
        CHECK(((em.prog.ops >> (2 * (em.n_ops - 1))) & 3u) == OP_ANDNOT, "a & ~heavy ends with ANDNOT");
        // below an OR, where the general emitter meets the ANDNOT: both sides as heavy, and b a leaf
        const SpecP mixed = bin_spec(Spec::OR, leaf_spec(5, false),
                                     bin_spec(Spec::ANDNOT, bin_spec(Spec::OR, leaf_spec(0, false), leaf_spec(1, false)),
                                              bin_spec(Spec::OR, leaf_spec(2, false), leaf_spec(3, false))));
        CHECK(check_tree(*mixed, tally, "or & ~or").ok, "or & ~or");
        const SpecP leafb = bin_spec(Spec::OR, leaf_spec(4, false),
                                     bin_spec(Spec::ANDNOT, bin_spec(Spec::OR, leaf_spec(0, false), leaf_spec(1, true)),
                                              leaf_spec(2, false)));
        CHECK(check_tree(*leafb, tally, "(x | y) & ~b").ok, "(x | y) & ~b");
        const SpecP plain = bin_spec(Spec::ANDNOT, leaf_spec(0, false), leaf_spec(1, false));
        const Emitter pe = check_tree(*plain, tally, "a & ~b");
        CHECK(pe.ok && eval_form(pe.prog) == FORM_CONJ && pe.prog.negate == 2u, "a & ~b: negate %u", pe.prog.negate);
    }
    {  // 9 leaves: refused, as postfix, DNF and CNF; 8: accepted
        Gen g(11);
        for (int n : {8, 9}) {
            g.next_id = 0;
            const SpecP conj = g.chain(n, Spec::AND);
            CHECK(check_tree(*conj, tally, "conjunction").ok == (n == 8), "conjunction of %d", n);
            g.next_id = 0;
            const SpecP ors = g.chain(n, Spec::OR);
            CHECK(check_tree(*ors, tally, "disjunction").ok == (n == 8), "disjunction of %d", n);
            for (const bool dnf : {true, false}) {
                // three groups of 3, 3 and n - 6 literals
                auto grp = [&](int first, int len) {
                    SpecP s = leaf_spec(first, false);
                    for (int i = 1; i < len; ++i)
                        s = bin_spec(dnf ? Spec::AND : Spec::OR, std::move(s), leaf_spec(first + i, i == 1));
                    return s;
                };
                const Spec::Kind outer = dnf ? Spec::OR : Spec::AND;
                const SpecP s = bin_spec(outer, bin_spec(outer, grp(0, 3), grp(3, 3)), grp(6, n - 6));
                const Emitter em = check_tree(*s, tally, dnf ? "dnf" : "cnf");
                CHECK(em.ok == (n == 8), "%s of %d literals: ok %d", dnf ? "dnf" : "cnf", n, (int)em.ok);
                if (n == 8)
                    CHECK(eval_form(em.prog) == (dnf ? FORM_DNF : FORM_CNF) && em.prog.gstart == 0x49u,
                          "two-level form %u gstart %x", eval_form(em.prog), em.prog.gstart);
            }
        }
    }
    {  // a single leaf, plain and complemented: one leaf, no op, emitted as postfix, run as a conjunction of one
        for (const bool neg : {false, true}) {
            const SpecP s = leaf_spec(3, neg);
            const Emitter em = check_tree(*s, tally, "single leaf");
            CHECK(em.ok && em.prog.n_leaves == 1 && em.prog.negate == (neg ? 1u : 0u) && em.prog.nops == 0 &&
                      em.max_depth == 1 && em.prog.form == FORM_POSTFIX && eval_form(em.prog) == FORM_CONJ,
                  "single leaf neg %d", (int)neg);
        }
    }
}

int run_trees(uint64_t n) {
    Tally dir;
    directed(dir);
    Tally t;
    const uint64_t per_seed = 5000;
    for (uint64_t done = 0, seed = 1; done < n; done += per_seed, ++seed) {
        Gen g(seed * 0x9e3779b97f4a7c15ull);
        fill_words(g.rng);
        for (uint64_t i = 0; i < per_seed && done + i < n; ++i) {
            const SpecP s = g.tree();
            CHECK(g.next_id <= kWords, "%d leaves", g.next_id);
            char what[64];
            std::snprintf(what, sizeof what, "seed %llu tree %llu", (unsigned long long)seed, (unsigned long long)i);
            check_tree(*s, t, what);
        }
    }
    std::printf("directed %llu\n", (unsigned long long)dir.trees);
    std::printf("trees %llu constant %llu accepted %llu deep %llu postfix %llu conj %llu dnf %llu cnf %llu\n",
                (unsigned long long)t.trees, (unsigned long long)t.constant, (unsigned long long)t.accepted,
                (unsigned long long)t.deep, (unsigned long long)t.form[FORM_POSTFIX],
                (unsigned long long)t.form[FORM_CONJ], (unsigned long long)t.form[FORM_DNF],
                (unsigned long long)t.form[FORM_CNF]);
    return 0;
}

// ---------------------------------------------------------------- algebra

int run_algebra() {
    Rng rng(3);
    fill_words(rng);
    Gen g(5);
    const Expr::Kind kinds[3] = {Expr::AND, Expr::OR, Expr::ANDNOT};
    auto apply = [](Expr::Kind k, uint64_t a, uint64_t b) { return k == Expr::AND ? (a & b) : k == Expr::OR ? (a | b) : (a & ~b); };
    uint64_t folded = 0;
    for (int i = 0; i < 2000; ++i) {
        g.next_id = 0;
        const SpecP s = g.any(1 + (int)g.below(10));
        const ExprP e = build(*s);
        const uint64_t v = value_of(*s);
        CHECK(value_of(e) == v, "tree %d", i);
        const ExprP n = mk_not(e), nn = mk_not(n);
        check_folded(n);
        check_folded(nn);
        CHECK(value_of(n) == ~v && value_of(nn) == v, "tree %d: NOT", i);
        CHECK(is_const(n) == is_const(e) && count_leaves(n) == count_leaves(e) && count_leaves(nn) == count_leaves(e),
              "tree %d: NOT changes the leaves", i);
        // a constant on either side, all three ops: the truth table, and a constant node exactly when
        // the value no longer depends on e
        for (const Expr::Kind k : kinds)
            for (const bool c : {false, true})
                for (const bool left : {false, true}) {
                    const ExprP cn = c ? mk_true() : mk_false();
                    const ExprP r = left ? mk_bin(k, cn, e) : mk_bin(k, e, cn);
                    const uint64_t cv = c ? ~0ull : 0ull;
                    CHECK(value_of(r) == (left ? apply(k, cv, v) : apply(k, v, cv)), "tree %d: op %d const %d left %d", i,
                          (int)k, (int)c, (int)left);
                    check_folded(r);
                    // the value is constant in e exactly when it is the same at e = 0 and e = ~0
                    const bool constant = is_const(e) || (left ? apply(k, cv, 0) == apply(k, cv, ~0ull)
                                                                : apply(k, 0, cv) == apply(k, ~0ull, cv));
                    CHECK(is_const(r) == constant, "tree %d: op %d const %d left %d: constant node %d", i, (int)k, (int)c,
                          (int)left, (int)is_const(r));
                    folded += is_const(r);
                }
    }
    // both sides constant: the eight truth-table rows of each op
    for (const Expr::Kind k : kinds)
        for (const bool a : {false, true})
            for (const bool b : {false, true}) {
                const ExprP r = mk_bin(k, a ? mk_true() : mk_false(), b ? mk_true() : mk_false());
                CHECK(is_const(r) && value_of(r) == apply(k, a ? ~0ull : 0ull, b ? ~0ull : 0ull), "op %d of %d, %d", (int)k,
                      (int)a, (int)b);
            }
    std::printf("algebra ok, %llu folded\n", (unsigned long long)folded);
    return 0;
}

// ---------------------------------------------------------------- postfix parser

int run_parser() {
    Rng rng(17);
    fill_words(rng);
    const uint64_t* leaves[32];
    for (int i = 0; i < 32; ++i) leaves[i] = &g_words[i];
    const int32_t opcodes[3] = {CUBIT_OP_AND, CUBIT_OP_OR, CUBIT_OP_ANDNOT};
    uint64_t accepted = 0;
    for (int it = 0; it < 20000; ++it) {
        // a random valid program over n_leaves slots (a leaf may appear twice), with its direct stack value
        const uint32_t n_leaves = 1 + (uint32_t)(rng() % 32), negate = (uint32_t)rng();
        const int pushes = 1 + (int)(rng() % 12);
        std::vector<int32_t> prog;
        std::vector<uint64_t> st;
        int pushed = 0;
        while (pushed < pushes || st.size() > 1) {
            if (pushed < pushes && (st.size() < 2 || rng() % 2)) {
                const uint32_t x = (uint32_t)(rng() % n_leaves);
                prog.push_back((int32_t)x);
                st.push_back(((negate >> x) & 1u) ? ~g_words[x] : g_words[x]);
                ++pushed;
            } else {
                const int32_t op = opcodes[rng() % 3];
                prog.push_back(op);
                const uint64_t b = st.back();
                st.pop_back();
                const uint64_t a = st.back();
                st.pop_back();
                st.push_back(op == CUBIT_OP_AND ? (a & b) : op == CUBIT_OP_OR ? (a | b) : (a & ~b));
            }
        }
        // heap copy at exact size: a read past the program is seen
        std::unique_ptr<int32_t[]> heap(new int32_t[prog.size()]);
        std::memcpy(heap.get(), prog.data(), prog.size() * sizeof(int32_t));
        const PostfixParse r = parse_postfix(leaves, n_leaves, negate, heap.get(), (uint32_t)prog.size());
        CHECK(r.error == PostfixParse::kNone && r.expr, "program %d refused: %d", it, (int)r.error);
        CHECK(value_of(r.expr) == st[0] && count_leaves(r.expr) == pushes, "program %d", it);
        ++accepted;
        // the same program with one malformation each
        const uint32_t n = (uint32_t)prog.size();
        {  // leaf index >= n_leaves, at a leaf's place
            std::vector<int32_t> bad = prog;
            uint32_t at = 0;
            while (bad[at] < 0) ++at;
            bad[at] = (int32_t)n_leaves + (int32_t)(rng() % 3);
            const PostfixParse b = parse_postfix(leaves, n_leaves, negate, bad.data(), n);
            CHECK(b.error == PostfixParse::kLeafRange && !b.expr && b.at == at && b.value == bad[at], "leaf range: %d", (int)b.error);
        }
        {  // an op before two values
            std::vector<int32_t> bad = prog;
            bad.insert(bad.begin() + 1, CUBIT_OP_OR);
            const PostfixParse b = parse_postfix(leaves, n_leaves, negate, bad.data(), n + 1);
            CHECK(b.error == PostfixParse::kUnderflow && !b.expr && b.at == 1, "underflow: %d at %u", (int)b.error, b.at);
        }
        {  // one more leaf: two values left
            std::vector<int32_t> bad = prog;
            bad.push_back(0);
            const PostfixParse b = parse_postfix(leaves, n_leaves, negate, bad.data(), n + 1);
            CHECK(b.error == PostfixParse::kLeftOver && !b.expr && b.left == 2, "left over: %d, %zu", (int)b.error, b.left);
        }
        if (n > 1) {  // an opcode outside CUBIT_OP_*, with two values under it
            std::vector<int32_t> bad = prog;
            bad[n - 1] = rng() % 2 ? -4 : INT32_MIN;
            const PostfixParse b = parse_postfix(leaves, n_leaves, negate, bad.data(), n);
            CHECK(b.error == PostfixParse::kBadOpcode && !b.expr && b.at == n - 1 && b.value == bad[n - 1], "opcode: %d", (int)b.error);
        }
    }
    const PostfixParse none = parse_postfix(leaves, 4, 0, nullptr, 0);
    CHECK(none.error == PostfixParse::kEmpty && !none.expr && none.left == 0, "empty program: %d", (int)none.error);
    const int32_t lone_op[1] = {CUBIT_OP_AND};
    CHECK(parse_postfix(leaves, 4, 0, lone_op, 1).error == PostfixParse::kUnderflow, "a lone op");
    const int32_t bad_lone[1] = {-9};  // underflow is checked before the opcode
    CHECK(parse_postfix(leaves, 4, 0, bad_lone, 1).error == PostfixParse::kUnderflow, "a lone bad opcode");
    std::printf("parser ok, %llu programs\n", (unsigned long long)accepted);
    return 0;
}

// ---------------------------------------------------------------- filter-tree walk

// a random filter tree in prefix order
void gen_filter(Rng& rng, int depth, std::vector<cubit_filter_node>& out) {
    cubit_filter_node f;
    std::memset(&f, 0, sizeof f);
    if (depth < 4 && rng() % 3 == 0) {
        f.kind = rng() % 2 ? CUBIT_FILTER_AND : CUBIT_FILTER_OR;
        f.n_children = (int32_t)(rng() % 4);  // 0 children included
        out.push_back(f);
        for (int k = 0; k < f.n_children; ++k) gen_filter(rng, depth + 1, out);
    } else {
        f.kind = (int32_t)(rng() % 3);  // CONSTANT, IS_NULL, IS_NOT_NULL
        f.cmp = (int32_t)(rng() % 6);
        f.column = (int32_t)(rng() % 5);
        f.constant = (int64_t)rng();
        out.push_back(f);
    }
}
// the walk, written recursively here
int64_t walk(const std::vector<cubit_filter_node>& v, size_t i) {
    if (i >= v.size()) return -1;
    size_t j = i + 1;
    for (int k = 0; k < v[i].n_children; ++k) {
        const int64_t e = walk(v, j);
        if (e < 0) return -1;
        j = (size_t)e;
    }
    return (int64_t)j;
}

int run_walk() {
    Rng rng(23);
    uint64_t arrays = 0, cuts = 0;
    for (int it = 0; it < 3000; ++it) {
        std::vector<cubit_filter_node> v;
        gen_filter(rng, it % 3 == 0 ? 0 : 2, v);
        const uint32_t n = (uint32_t)v.size();
        for (uint32_t len = 0; len <= n; ++len) {
            // heap copy at exact size: a read past a truncation is seen
            std::unique_ptr<cubit_filter_node[]> heap(new cubit_filter_node[len]);
            if (len) std::memcpy(heap.get(), v.data(), len * sizeof(cubit_filter_node));
            const int end = filter_subtree_end(heap.get(), len, 0);
            if (len == n) CHECK(end == (int)n, "array %d: end %d of %u", it, end, n);
            else CHECK(end == -1, "array %d cut to %u of %u: end %d", it, len, n, end);
            cuts += len < n;
        }
        // every inner subtree ends where the recursive walk says, and one past the array is refused
        for (uint32_t i = 0; i < n; ++i) CHECK(filter_subtree_end(v.data(), n, i) == (int)walk(v, i), "array %d node %u", it, i);
        CHECK(filter_subtree_end(v.data(), n, n) == -1, "array %d: a start past the end", it);
        ++arrays;
    }
    {  // a child count past the array, and a negative one (reads as none)
        cubit_filter_node f[2];
        std::memset(f, 0, sizeof f);
        f[0].kind = CUBIT_FILTER_AND;
        f[0].n_children = INT32_MAX;
        CHECK(filter_subtree_end(f, 2, 0) == -1, "INT32_MAX children");
        f[0].n_children = -3;
        CHECK(filter_subtree_end(f, 2, 0) == 1, "negative children");
    }
    // the node check: kind in CONSTANT … AND, cmp in 0 … 5 on a constant filter only
    for (int32_t kind = -2; kind <= 7; ++kind)
        for (int32_t cmp = -2; cmp <= 8; ++cmp) {
            cubit_filter_node f;
            std::memset(&f, 0, sizeof f);
            f.kind = kind;
            f.cmp = cmp;
            const NodeCheck want = kind < CUBIT_FILTER_CONSTANT || kind > CUBIT_FILTER_AND ? NodeCheck::kBadKind
                                   : kind == CUBIT_FILTER_CONSTANT && (cmp < 0 || cmp > 5)  ? NodeCheck::kBadCmp
                                                                                            : NodeCheck::kOk;
            CHECK(check_filter_node(f) == want, "kind %d cmp %d", kind, cmp);
        }
    for (const int32_t kind : {INT32_MIN, INT32_MAX}) {
        cubit_filter_node f;
        std::memset(&f, 0, sizeof f);
        f.kind = kind;
        CHECK(check_filter_node(f) == NodeCheck::kBadKind, "kind %d", kind);
    }
    std::printf("walk ok, %llu arrays, %llu truncations\n", (unsigned long long)arrays, (unsigned long long)cuts);
    return 0;
}

// ---------------------------------------------------------------- CmpRange

bool compare(int cmp, int64_t v, int64_t c, int64_t c2) {
    switch (cmp) {
    case CUBIT_CMP_EQ: return v == c;
    case CUBIT_CMP_NE: return v != c;
    case CUBIT_CMP_LT: return v < c;
    case CUBIT_CMP_LE: return v <= c;
    case CUBIT_CMP_GT: return v > c;
    case CUBIT_CMP_GE: return v >= c;
    default: return c <= v && v < c2;  // the between form
    }
}

int run_range() {
    const int64_t edge[7] = {INT64_MIN, INT64_MIN + 1, -1, 0, 1, INT64_MAX - 1, INT64_MAX};
    const int64_t edge32[9] = {INT32_MIN, (int64_t)INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX,
                               (int64_t)INT32_MIN - 1, (int64_t)INT32_MAX + 1};
    struct Case {
        int cmp;
        int64_t c, c2;
    };
    std::vector<Case> cases;
    for (int cmp = 0; cmp <= 5; ++cmp)
        for (const int64_t c : edge) cases.push_back({cmp, c, 0});
    for (const int64_t c : edge)
        for (const int64_t c2 : edge) cases.push_back({6, c, c2});
    for (const int64_t c : edge32)  // constants around the INT32 edges, for clamp32
        for (int cmp = 0; cmp <= 5; ++cmp) cases.push_back({cmp, c, 0});
    uint64_t pairs = 0;
    for (const Case& a : cases) {
        const CmpRange r = cmp_range(a.cmp, a.c, a.c2);
        CHECK((r.neg != 0) == (a.cmp == CUBIT_CMP_NE), "cmp %d: neg %d", a.cmp, r.neg);
        bool any = false, any32 = false;
        for (const int64_t v : edge) {
            const bool want = compare(a.cmp, v, a.c, a.c2);
            CHECK(r.contains(v) == want, "cmp %d c %lld c2 %lld v %lld", a.cmp, (long long)a.c, (long long)a.c2, (long long)v);
            any |= want != (r.neg != 0);
        }
        // the range before the complement is empty exactly when no value is inside (its own ends are the witnesses)
        if (!r.empty()) CHECK(compare(a.cmp, r.lo, a.c, a.c2) != (r.neg != 0) && compare(a.cmp, r.hi, a.c, a.c2) != (r.neg != 0), "ends of cmp %d", a.cmp);
        else CHECK(!any, "cmp %d c %lld: empty range with a member", a.cmp, (long long)a.c);
        // clamp32: the same members among the INT32 values, and empty when the range misses INT32
        int32_t lo32, hi32;
        r.clamp32(lo32, hi32);
        for (const int64_t v : edge32) {
            if (v < INT32_MIN || v > INT32_MAX) continue;
            const bool in32 = (int32_t)v >= lo32 && (int32_t)v <= hi32;
            CHECK((in32 != (r.neg != 0)) == compare(a.cmp, v, a.c, a.c2), "clamp32 cmp %d c %lld v %lld", a.cmp, (long long)a.c, (long long)v);
            any32 |= in32;
        }
        if (r.empty() || r.lo > INT32_MAX || r.hi < INT32_MIN) CHECK(lo32 > hi32 && !any32, "clamp32 of a range outside INT32");
        else CHECK(lo32 <= hi32 && lo32 == std::max<int64_t>(r.lo, INT32_MIN) && hi32 == std::min<int64_t>(r.hi, INT32_MAX), "clamp32 ends");
        // intersection = conjunction (ranges that are not complemented: != is no range)
        if (r.neg) continue;
        for (const Case& b : cases) {
            const CmpRange s = cmp_range(b.cmp, b.c, b.c2);
            if (s.neg) continue;
            const CmpRange both = r.intersect(s);
            CHECK(both.neg == 0, "intersection complemented");
            for (const int64_t v : edge)
                CHECK(both.contains(v) == (compare(a.cmp, v, a.c, a.c2) && compare(b.cmp, v, b.c, b.c2)),
                      "cmp %d c %lld and cmp %d c %lld at %lld", a.cmp, (long long)a.c, b.cmp, (long long)b.c, (long long)v);
            CHECK(both.empty() == !(both.lo <= both.hi), "empty()");
            if (!both.empty()) CHECK(r.contains(both.lo) && s.contains(both.lo) && r.contains(both.hi) && s.contains(both.hi), "ends of an intersection");
            ++pairs;
        }
    }
    std::printf("range ok, %zu comparisons, %llu pairs\n", cases.size(), (unsigned long long)pairs);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "trees" && argc > 2) return run_trees(std::strtoull(argv[2], nullptr, 10));
    if (mode == "algebra") return run_algebra();
    if (mode == "parser") return run_parser();
    if (mode == "walk") return run_walk();
    if (mode == "range") return run_range();
    std::printf("usage: program_core trees N | algebra | parser | walk | range\n");
    return 2;
}
