// onnx_proto.h -- the ONNX protobuf decoding shared by the two model readers: the family reader
// (onnx_reader.cc, ONNX -> NSGW) and the general graph planner (onnx_graph.cc).
//
// The protobuf wire format is decoded by hand from the public onnx.proto3 field numbers (no
// protobuf / onnx dependency).  Every malformed or truncated input throws nsg::onnx::wire::Error.
#ifndef NSG_ONNX_PROTO_H
#define NSG_ONNX_PROTO_H

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace nsg {
namespace onnx {
namespace wire {

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// ---- protobuf wire format -------------------------------------------------------------------
struct Span {
    const unsigned char* p = nullptr;
    size_t n = 0;
};

struct Field {
    uint32_t number = 0;
    int wire = 0;
    uint64_t value = 0; // varint / fixed
    Span bytes;         // length-delimited, fixed32, fixed64
};

class Reader {
 public:
    explicit Reader(Span S) : P(S.p), End(S.p + S.n) {}
    bool next(Field* F) {
        if (P >= End) return false;
        const uint64_t Key = varint();
        F->number = (uint32_t)(Key >> 3);
        F->wire = (int)(Key & 7);
        F->value = 0;
        F->bytes = Span{}; // a varint field must not leave the previous field's bytes behind
        switch (F->wire) {
        case 0: F->value = varint(); break;
        case 1: F->bytes = take(8); break;
        case 2: F->bytes = take((size_t)varint()); break;
        case 5: F->bytes = take(4); break;
        default: throw Error("unsupported protobuf wire type " + std::to_string(F->wire));
        }
        return true;
    }
    uint64_t varint() {
        uint64_t V = 0;
        for (int Shift = 0; Shift < 70; Shift += 7) {
            if (P >= End) throw Error("truncated protobuf varint");
            const unsigned char B = *P++;
            V |= (uint64_t)(B & 0x7F) << Shift;
            if (!(B & 0x80)) return V;
        }
        throw Error("malformed protobuf varint");
    }
    bool done() const { return P >= End; }

 private:
    Span take(size_t N) {
        if ((size_t)(End - P) < N) throw Error("truncated protobuf field");
        Span S{P, N};
        P += N;
        return S;
    }
    const unsigned char* P;
    const unsigned char* End;
};

inline std::string str(Span S) { return std::string((const char*)S.p, S.n); }

inline float f32(Span S) {
    if (!S.p || S.n < 4) throw Error("malformed protobuf: a float field is not 4 bytes wide");
    float V;
    std::memcpy(&V, S.p, 4);
    return V;
}

inline double f64(Span S) {
    if (!S.p || S.n < 8) throw Error("malformed protobuf: a double field is not 8 bytes wide");
    double V;
    std::memcpy(&V, S.p, 8);
    return V;
}

// a field that must be length-delimited (strings, sub-messages, raw_data)
inline Span bytesOf(const Field& F, const char* What) {
    if (F.wire != 2) throw Error(std::string("malformed protobuf: ") + What + " is not length-delimited");
    return F.bytes;
}

// ---- ONNX messages (onnx.proto3 field numbers) ----------------------------------------------
struct Tensor {
    std::vector<int64_t> Dims;
    std::vector<float> F;   // data_type FLOAT (1); DOUBLE (11) is rounded to float on reading
    std::vector<int64_t> I; // data_type INT64 (7)
    bool IsFloat = true;
    size_t count() const { return IsFloat ? F.size() : I.size(); }
};

inline Tensor readTensor(Span S, std::string* Name) {
    Tensor T;
    int DataType = 0;
    Span Raw;
    bool HasRaw = false;
    std::vector<double> Doubles;
    Reader R(S);
    Field Fd;
    while (R.next(&Fd)) {
        switch (Fd.number) {
        case 1: // dims
            if (Fd.wire == 0) T.Dims.push_back((int64_t)Fd.value);
            else { Reader P(Fd.bytes); while (!P.done()) T.Dims.push_back((int64_t)P.varint()); }
            break;
        case 2: DataType = (int)Fd.value; break;
        case 4: // float_data
            if (Fd.wire == 5) T.F.push_back(f32(Fd.bytes));
            else if (Fd.wire == 2) for (size_t K = 0; K + 4 <= Fd.bytes.n; K += 4) T.F.push_back(f32(Span{Fd.bytes.p + K, 4}));
            else throw Error("malformed protobuf: float_data is neither fixed32 nor packed");
            break;
        case 7: // int64_data
            if (Fd.wire == 0) T.I.push_back((int64_t)Fd.value);
            else { Reader P(Fd.bytes); while (!P.done()) T.I.push_back((int64_t)P.varint()); }
            break;
        case 8: if (Name) *Name = str(bytesOf(Fd, "a tensor name")); break;
        case 10: // double_data
            if (Fd.wire == 1) Doubles.push_back(f64(Fd.bytes));
            else if (Fd.wire == 2) for (size_t K = 0; K + 8 <= Fd.bytes.n; K += 8) Doubles.push_back(f64(Span{Fd.bytes.p + K, 8}));
            else throw Error("malformed protobuf: double_data is neither fixed64 nor packed");
            break;
        case 9: Raw = bytesOf(Fd, "raw_data"); HasRaw = true; break;
        case 14: if (Fd.value != 0) throw Error("initializer with external data: not supported (keep the weights inside the .onnx file)"); break;
        default: break;
        }
    }
    if (DataType == 1) {
        T.IsFloat = true;
        if (HasRaw) {
            T.F.resize(Raw.n / 4);
            std::memcpy(T.F.data(), Raw.p, T.F.size() * 4);
        }
    } else if (DataType == 11) { // torch writes a Python float literal (clamp's bound) as a double constant behind a Cast
        T.IsFloat = true;
        if (HasRaw) {
            Doubles.resize(Raw.n / 8);
            std::memcpy(Doubles.data(), Raw.p, Doubles.size() * 8);
        }
        T.F.assign(Doubles.begin(), Doubles.end());
    } else if (DataType == 7) {
        T.IsFloat = false;
        if (HasRaw) {
            T.I.resize(Raw.n / 8);
            std::memcpy(T.I.data(), Raw.p, T.I.size() * 8);
        }
    } else {
        throw Error("initializer '" + (Name ? *Name : std::string()) + "': unsupported data type " +
                    std::to_string(DataType) + " (float32 / float64 / int64 only)");
    }
    size_t Want = 1;
    for (int64_t D : T.Dims) Want *= (size_t)D;
    if (Want != T.count()) throw Error("initializer '" + (Name ? *Name : std::string()) + "': element count does not match its dims");
    return T;
}

struct Attr {
    bool HasF = false, HasI = false;
    float F = 0.f;
    int64_t I = 0;
    std::vector<int64_t> Ints;
    std::shared_ptr<Tensor> T;
};

struct Node {
    std::string Op, Name;
    std::vector<std::string> In, Out;
    std::map<std::string, Attr> Attrs;
    int64_t attrI(const char* K, int64_t Default) const {
        auto It = Attrs.find(K);
        return It != Attrs.end() && It->second.HasI ? It->second.I : Default;
    }
    double attrF(const char* K, double Default) const {
        auto It = Attrs.find(K);
        return It != Attrs.end() && It->second.HasF ? (double)It->second.F : Default;
    }
    std::vector<int64_t> attrInts(const char* K, std::vector<int64_t> Default) const {
        auto It = Attrs.find(K);
        return It != Attrs.end() && !It->second.Ints.empty() ? It->second.Ints : Default;
    }
};

inline Node readNode(Span S) {
    Node N;
    Reader R(S);
    Field Fd;
    while (R.next(&Fd)) {
        switch (Fd.number) {
        case 1: N.In.push_back(str(bytesOf(Fd, "a node input"))); break;
        case 2: N.Out.push_back(str(bytesOf(Fd, "a node output"))); break;
        case 3: N.Name = str(bytesOf(Fd, "a node name")); break;
        case 4: N.Op = str(bytesOf(Fd, "an op type")); break;
        case 5: {
            std::string Name;
            Attr A;
            Reader AR(bytesOf(Fd, "an attribute"));
            Field Af;
            while (AR.next(&Af)) {
                switch (Af.number) {
                case 1: Name = str(bytesOf(Af, "an attribute name")); break;
                case 2:
                    if (Af.wire != 5) throw Error("malformed protobuf: attribute float is not fixed32");
                    A.F = f32(Af.bytes); A.HasF = true; break;
                case 3: A.I = (int64_t)Af.value; A.HasI = true; break;
                case 5: A.T = std::make_shared<Tensor>(readTensor(bytesOf(Af, "an attribute tensor"), nullptr)); break;
                case 8:
                    if (Af.wire == 0) A.Ints.push_back((int64_t)Af.value);
                    else { Reader P(Af.bytes); while (!P.done()) A.Ints.push_back((int64_t)P.varint()); }
                    break;
                default: break;
                }
            }
            N.Attrs[Name] = A;
            break;
        }
        default: break;
        }
    }
    return N;
}

inline std::string valueInfoName(Span S) {
    Reader R(S);
    Field Fd;
    while (R.next(&Fd))
        if (Fd.number == 1) return str(bytesOf(Fd, "a value-info name"));
    return std::string();
}

struct Graph {
    std::vector<Node> Nodes;
    std::map<std::string, Tensor> Inits;
    std::vector<std::string> Inputs, Outputs;
    std::vector<Span> InputInfos, OutputInfos; // the ValueInfoProto bytes of each (inside the model buffer)
    std::map<std::string, std::vector<const Node*>> Consumers;
};

inline Graph readModel(Span Data) {
    Span GraphBytes;
    bool HaveGraph = false;
    {
        Reader R(Data);
        Field Fd;
        while (R.next(&Fd))
            if (Fd.number == 7 && Fd.wire == 2) { GraphBytes = Fd.bytes; HaveGraph = true; }
    }
    if (!HaveGraph) throw Error("not an ONNX ModelProto: no graph");
    Graph G;
    Reader R(GraphBytes);
    Field Fd;
    while (R.next(&Fd)) {
        if (Fd.wire != 2) continue;
        if (Fd.number == 1) G.Nodes.push_back(readNode(Fd.bytes));
        else if (Fd.number == 5) { std::string Name; Tensor T = readTensor(Fd.bytes, &Name); G.Inits[Name] = std::move(T); }
        else if (Fd.number == 11) { G.Inputs.push_back(valueInfoName(Fd.bytes)); G.InputInfos.push_back(Fd.bytes); }
        else if (Fd.number == 12) { G.Outputs.push_back(valueInfoName(Fd.bytes)); G.OutputInfos.push_back(Fd.bytes); }
    }
    // Constant nodes are initializers in all but name (torch emits them for scalar literals)
    for (const Node& N : G.Nodes) {
        if (N.Op != "Constant" || N.Out.size() != 1) continue;
        auto It = N.Attrs.find("value");
        if (It != N.Attrs.end() && It->second.T) G.Inits[N.Out[0]] = *It->second.T;
        else if ((It = N.Attrs.find("value_float")) != N.Attrs.end() && It->second.HasF) {
            Tensor T;
            T.F.push_back(It->second.F);
            G.Inits[N.Out[0]] = T;
        }
    }
    for (const Node& N : G.Nodes)
        for (const std::string& I : N.In) G.Consumers[I].push_back(&N);
    return G;
}

// Declared dims of a ValueInfoProto (type.tensor_type.shape): a symbolic or missing dim is -1.  Returns false when
// the value info carries no shape.
inline bool valueInfoDims(Span S, std::vector<int64_t>* Dims) {
    Dims->clear();
    bool Have = false;
    Reader R(S);
    Field Fd;
    while (R.next(&Fd)) {
        if (Fd.number != 2 || Fd.wire != 2) continue; // type
        Reader T(Fd.bytes);
        Field Tf;
        while (T.next(&Tf)) {
            if (Tf.number != 1 || Tf.wire != 2) continue; // tensor_type
            Reader TT(Tf.bytes);
            Field Sf;
            while (TT.next(&Sf)) {
                if (Sf.number != 2 || Sf.wire != 2) continue; // shape
                Have = true;
                Reader SR(Sf.bytes);
                Field Df;
                while (SR.next(&Df)) {
                    if (Df.number != 1 || Df.wire != 2) continue; // dim
                    int64_t V = -1;
                    Reader DR(Df.bytes);
                    Field Vf;
                    while (DR.next(&Vf))
                        if (Vf.number == 1 && Vf.wire == 0) V = (int64_t)Vf.value;
                    Dims->push_back(V);
                }
            }
        }
    }
    return Have;
}

} // namespace wire
} // namespace onnx
} // namespace nsg

#endif
