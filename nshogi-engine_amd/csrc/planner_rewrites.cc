// planner_rewrites.cc -- the planner: pattern rewrites on the node list.
#include "planner.h"

namespace nsg::graph {

namespace {

constexpr int kAnyArity = -1;

// What the patterns share: the live nodes' consumer counts and producers, and the questions a pattern asks of them.
// The patterns were written at different times and accept slightly different things; each keeps what it accepted:
//   * erf-GELU compares 0.5 and 1.0 exactly and sqrt(2) within 1e-6; Mish, tanh-GELU and softsign compare their
//     constants as f32 within one ulp (near).
//   * erf-GELU's interior nodes are taken whatever their arity and without a look at Skip (inner with kAnyArity), and
//     it counts the consumers again after each match (count); the others check both and count once.
//   * erf-GELU takes the first scalar operand of a node and then looks at its value; the others take the first operand
//     that is the scalar they want.
//   * swish keeps its node's name; the others prefix the absorbed nodes' names, erf-GELU in the pattern's order, the
//     rest in node order.
struct Matcher {
    std::vector<Node>& Nodes;
    std::vector<bool>& Skip;
    const std::map<std::string, Tensor>& Inits;
    const std::set<std::string>& Outputs;
    std::map<std::string, int> Cnt;         // consumers among the live nodes
    std::map<std::string, size_t> Producer; // tensor -> the live node that computes it

    void count() {
        Cnt.clear();
        for (size_t K = 0; K < Nodes.size(); ++K)
            if (!Skip[K])
                for (const std::string& I : Nodes[K].In) ++Cnt[I];
    }
    void index() {
        count();
        Producer.clear();
        for (size_t K = 0; K < Nodes.size(); ++K)
            if (!Skip[K])
                for (const std::string& O : Nodes[K].Out) Producer[O] = K;
    }
    // the node producing the interior tensor T (one consumer, no graph output) when it has op `Op`, or -1
    int inner(const std::string& T, const char* Op, int Arity) const {
        auto It = Producer.find(T);
        if (It == Producer.end() || Nodes[It->second].Op != Op) return -1;
        if (Arity != kAnyArity && (Skip[It->second] || Nodes[It->second].In.size() != (size_t)Arity)) return -1;
        auto C = Cnt.find(T);
        if (C == Cnt.end() || C->second != 1 || Outputs.count(T)) return -1;
        return (int)It->second;
    }
    bool scalar(const std::string& T, double* V) const {
        auto It = Inits.find(T);
        if (It == Inits.end() || !It->second.IsFloat || It->second.F.size() != 1) return false;
        *V = It->second.F[0];
        return true;
    }
    // the other operand of the two-input node I, beside the first operand that is a scalar constant `Accept` takes
    template <class Fn> bool beside(int I, Fn Accept, std::string* Other) const {
        const Node& N = Nodes[(size_t)I];
        if (N.In.size() != 2) return false;
        double V = 0;
        for (int Side = 0; Side < 2; ++Side)
            if (scalar(N.In[(size_t)Side], &V) && Accept(V)) { *Other = N.In[(size_t)(1 - Side)]; return true; }
        return false;
    }
    // the other operand of the two-input node I, one of whose operands is T
    bool partner(int I, const std::string& T, std::string* Other) const {
        const Node& N = Nodes[(size_t)I];
        for (int Side = 0; Side < 2; ++Side)
            if (N.In[(size_t)Side] == T && N.In[(size_t)(1 - Side)] != T) { *Other = N.In[(size_t)(1 - Side)]; return true; }
        return false;
    }
    // node K becomes Op(X); the absorbed nodes are skipped, their names in the order given go before K's
    void become(size_t K, const char* Op, std::string X, const std::vector<int>& Absorbed, bool Named = true) {
        Node& N = Nodes[K];
        std::string Name;
        for (int I : Absorbed) {
            Skip[(size_t)I] = true;
            if (Named) Name += Nodes[(size_t)I].Name + "+";
        }
        N.Name = Name + N.Name;
        N.Op = Op;
        N.In = {std::move(X)};
    }
};

std::vector<int> inNodeOrder(std::vector<int> V) {
    std::sort(V.begin(), V.end());
    return V;
}

// f32 within one ulp
auto near(double Want) {
    return [Want](double V) {
        const float A = (float)V, B = (float)Want;
        return A == B || A == std::nextafterf(B, 0.f) || A == std::nextafterf(B, 2.f * B);
    };
}

// Mul(x, Sigmoid(x)) -> Swish(x) when the Sigmoid feeds only the Mul
void swish(Matcher& M) {
    for (size_t K = 0; K < M.Nodes.size(); ++K) {
        const Node& N = M.Nodes[K];
        if (N.Op != "Mul" || N.In.size() != 2) continue;
        for (int Side = 0; Side < 2; ++Side) {
            const std::string& X = N.In[(size_t)(1 - Side)];
            const int IS = M.inner(N.In[(size_t)Side], "Sigmoid", 1);
            if (IS < 0 || M.Nodes[(size_t)IS].In[0] != X) continue;
            M.become(K, "Swish", X, {IS}, false);
            break;
        }
    }
}

// The exact GELU as the exporter writes it, x * (1 + erf(x / sqrt(2))) * 0.5 over five nodes, becomes one Gelu node
// (then an activation like any other: it fuses into a dense epilogue).
void erfGelu(Matcher& M) {
    std::vector<Node>& Nodes = M.Nodes;
    double V = 0;
    auto any = [&V](double S) { V = S; return true; };
    for (size_t K = 0; K < Nodes.size(); ++K) {
        std::string T1, T2, T3;
        if (M.Skip[K] || Nodes[K].Op != "Mul" || !M.beside((int)K, any, &T1) || V != 0.5) continue;
        const int IM = M.inner(T1, "Mul", kAnyArity); // x * (erf + 1)
        if (IM < 0 || Nodes[(size_t)IM].In.size() != 2) continue;
        for (int Side = 0; Side < 2; ++Side) {
            const std::string& X = Nodes[(size_t)IM].In[(size_t)Side];
            const int IA = M.inner(Nodes[(size_t)IM].In[(size_t)(1 - Side)], "Add", kAnyArity);
            if (IA < 0 || !M.beside(IA, any, &T2) || V != 1.0) continue;
            const int IE = M.inner(T2, "Erf", kAnyArity);
            if (IE < 0 || Nodes[(size_t)IE].In.size() != 1) continue;
            const int ID = M.inner(Nodes[(size_t)IE].In[0], "Div", kAnyArity);
            const int IS = M.inner(Nodes[(size_t)IE].In[0], "Mul", kAnyArity);
            const int IX = ID >= 0 ? ID : IS;
            if (IX < 0 || !M.beside(IX, any, &T3) || T3 != X) continue;
            if (ID >= 0 && (Nodes[(size_t)ID].In[0] != X || std::fabs(V - std::sqrt(2.0)) > 1e-6)) continue;
            if (ID < 0 && std::fabs(V - std::sqrt(0.5)) > 1e-6) continue;
            M.become(K, "Gelu", X, {IX, IE, IA, IM});
            M.count(); // the counts the next candidate sees
            break;
        }
    }
}

// Mish, tanh-GELU and softsign as the exporter writes them become one node each (MishAct, GeluTanh, Softsign), then an
// activation like any other.  x is the one tensor a pattern reads more than once; every other tensor inside has one
// consumer and is no graph output; commutative nodes match in either operand order.  A chain that starts like a
// pattern and then deviates is left as it is: plain elementwise nodes.
//   Mish       Mul(x, Tanh(Softplus(x)))
//   tanh-GELU  Mul(Mul(x, Add(Tanh(Mul(Add(x, Mul(x^3, 0.044715)), sqrt(2/pi))), 1)), 0.5), the 0.5 on either Mul;
//              x^3 is Mul(Mul(x, x), x) or Pow(x, 3)
//   softsign   Div(x, Add(Abs(x), 1))
// x^3 of X as the tensor T: the nodes that compute it
bool cube(const Matcher& M, const std::string& T, const std::string& X, std::vector<int>* Absorbed) {
    const std::vector<Node>& Nodes = M.Nodes;
    double E = 0;
    const int IP = M.inner(T, "Pow", 2);
    if (IP >= 0) {
        if (Nodes[(size_t)IP].In[0] != X || !M.scalar(Nodes[(size_t)IP].In[1], &E) || !near(3.0)(E)) return false;
        Absorbed->push_back(IP);
        return true;
    }
    const int IM = M.inner(T, "Mul", 2);
    std::string Sq;
    if (IM < 0 || !M.partner(IM, X, &Sq)) return false;
    const int IS = M.inner(Sq, "Mul", 2);
    if (IS < 0 || Nodes[(size_t)IS].In[0] != X || Nodes[(size_t)IS].In[1] != X) return false;
    Absorbed->insert(Absorbed->end(), {IM, IS});
    return true;
}

// tanh(sqrt(2/pi) (x + 0.044715 x^3)) + 1 as the tensor T
bool geluTail(const Matcher& M, const std::string& T, const std::string& X, std::vector<int>* Absorbed) {
    std::string Th, Sum, Cb, X3;
    const int IA = M.inner(T, "Add", 2);
    if (IA < 0 || !M.beside(IA, near(1.0), &Th)) return false;
    const int IT = M.inner(Th, "Tanh", 1);
    if (IT < 0) return false;
    const int IK = M.inner(M.Nodes[(size_t)IT].In[0], "Mul", 2);
    if (IK < 0 || !M.beside(IK, near(0.7978845608028654), &Sum)) return false;
    const int IS = M.inner(Sum, "Add", 2);
    if (IS < 0 || !M.partner(IS, X, &Cb)) return false;
    const int IC = M.inner(Cb, "Mul", 2);
    if (IC < 0 || !M.beside(IC, near(0.044715), &X3) || !cube(M, X3, X, Absorbed)) return false;
    Absorbed->insert(Absorbed->end(), {IA, IT, IK, IS, IC});
    return true;
}

void mishGeluTanhSoftsign(Matcher& M) {
    std::vector<Node>& Nodes = M.Nodes;
    for (size_t K = 0; K < Nodes.size(); ++K) {
        const Node& N = Nodes[K];
        if (M.Skip[K] || N.In.size() != 2) continue;
        if (N.Op == "Div") { // softsign
            std::string Ab;
            const int IA = M.inner(N.In[1], "Add", 2);
            if (IA < 0 || !M.beside(IA, near(1.0), &Ab)) continue;
            const int IB = M.inner(Ab, "Abs", 1);
            if (IB < 0 || Nodes[(size_t)IB].In[0] != N.In[0]) continue;
            M.become(K, "Softsign", N.In[0], inNodeOrder({IA, IB}));
            continue;
        }
        if (N.Op != "Mul") continue;
        bool Done = false;
        for (int Side = 0; Side < 2 && !Done; ++Side) { // Mish: Mul(x, Tanh(Softplus(x)))
            const std::string X = N.In[(size_t)Side];
            const int IT = M.inner(N.In[(size_t)(1 - Side)], "Tanh", 1);
            if (IT < 0) continue;
            const int IS = M.inner(Nodes[(size_t)IT].In[0], "Softplus", 1);
            if (IS < 0 || Nodes[(size_t)IS].In[0] != X) continue;
            M.become(K, "MishAct", X, inNodeOrder({IT, IS}));
            Done = true;
        }
        if (Done) continue;
        // tanh-GELU: (x * tail) * 0.5, or (x * 0.5) * tail
        std::string Prod, X;
        if (M.beside((int)K, near(0.5), &Prod)) {
            const int IM = M.inner(Prod, "Mul", 2);
            for (int Side = 0; Side < 2 && IM >= 0 && !Done; ++Side) {
                std::vector<int> Absorbed = {IM};
                X = Nodes[(size_t)IM].In[(size_t)Side];
                if (!geluTail(M, Nodes[(size_t)IM].In[(size_t)(1 - Side)], X, &Absorbed)) continue;
                M.become(K, "GeluTanh", X, inNodeOrder(Absorbed));
                Done = true;
            }
            if (Done) continue;
        }
        for (int Side = 0; Side < 2 && !Done; ++Side) {
            const int IH = M.inner(N.In[(size_t)Side], "Mul", 2);
            if (IH < 0 || !M.beside(IH, near(0.5), &X)) continue;
            std::vector<int> Absorbed = {IH};
            if (!geluTail(M, N.In[(size_t)(1 - Side)], X, &Absorbed)) continue;
            M.become(K, "GeluTanh", X, inNodeOrder(Absorbed));
            Done = true;
        }
    }
}

} // namespace

void rewritePatterns(std::vector<Node>& Nodes, std::vector<bool>& Skip, const std::map<std::string, Tensor>& Inits,
                     const std::set<std::string>& Outputs) {
    Matcher M{Nodes, Skip, Inits, Outputs, {}, {}};
    for (void (*Pass)(Matcher&) : {swish, erfGelu, mishGeluTanhSoftsign}) {
        M.index();
        Pass(M);
    }
}

} // namespace nsg::graph
