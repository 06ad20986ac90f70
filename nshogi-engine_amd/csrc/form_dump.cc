// form_dump -- the launch form of every batch size of a fixed grid of configurations, as text
// (tests/test_launch_forms.py compares it with tests/golden/launch_forms.txt).  Links launch_form.cc alone.
//
//   == cus prec F cpad                      one section per device size, precision and network shape; "same as" an
//                                           earlier section when all that follows would equal that section's text
//   lo..hi form                             the section's first table: teamAvailable, coopAvailable, inside the M8
//                                           window (team=1 coop=1 outside=0), every knob at its default
//   -- variant, variant, ...                the other variants -- team / coop / outside, or the first table's
//                                           configuration with ONE knob of LaunchConfig / ConvTuning changed -- that
//                                           share the lines below them: the batch sizes whose form is NOT the first
//                                           table's, with their form (no lines: the variant changes nothing)
//                                           ("the lines of [section -- variant]": those printed there)
//   form = Kind nb/nfrag/nwaves [m] [k] [s] [mem] [stem1] [ch] [per] [stag1] prec L [| off+count plan prec]...
//                                           batch sizes lo..hi (1 .. 4 cus + 64) take this form: the plan with its row,
//                                           K and slab split where they are not 1; members, stemFirst, chains, per and stagger where they
//                                           are not 0, false, 1, 0 and false (perE: B / chains rounded up to whole
//                                           two-board tiles); trunkPrec ("own": the evaluator's precision),
//                                           trunkLaunchesPerFwd; then every part (the last one takes the rest)
#include "launch_form.h"

#include <cstdio>
#include <functional>
#include <map>
#include <string>
#include <utility>
#include <vector>

using namespace nsg;

namespace {

const char* const kPrecNames[] = {"fp32", "fp16", "bf16", "f16x3", "f16m8", "f16m6"};
const char* const kKindNames[] = {"Team", "Coop", "WholeTrunk", "Parts", "Chains", "Single"};

std::string planText(const ConvPlan& p) { // (a row, K or slab split of 1 is left out)
    char b[96];
    int n = snprintf(b, sizeof(b), "%d/%d/%d", p.nb, p.nfrag, p.nwaves);
    if (p.msplit != 1) n += snprintf(b + n, sizeof(b) - n, " m%d", p.msplit);
    if (p.ksplit != 1) n += snprintf(b + n, sizeof(b) - n, " k%d", p.ksplit);
    if (p.sslab != 1) n += snprintf(b + n, sizeof(b) - n, " s%d", p.sslab);
    return b;
}

std::string formText(const LaunchForm& f, int B, int ownPrec) {
    auto precName = [&](int p) { return p == ownPrec ? "own" : kPrecNames[p]; };
    char b[96];
    std::string s = std::string(kKindNames[f.kind]) + " " + planText(f.plan);
    auto field = [&](bool show, const char* fmt, int v) { if (show) { snprintf(b, sizeof(b), fmt, v); s += b; } };
    field(f.members != 0, " mem%d", f.members);
    field(f.stemFirst, " stem%d", 1);
    field(f.chains != 1, " ch%d", f.chains);
    // (perE: B / chains rounded up to whole two-board tiles, so that a run of batch sizes stays one line)
    if (f.kind == LaunchForm::Chains && f.per == ((B + f.chains - 1) / f.chains + 1) / 2 * 2) s += " perE";
    else field(f.per != 0, " per%d", f.per);
    field(f.stagger, " stag%d", 1);
    snprintf(b, sizeof(b), " %s L%d", precName(f.trunkPrec), f.trunkLaunchesPerFwd);
    s += b;
    for (int i = 0; i < f.nParts; ++i) {
        // (the last part is the rest of the batch: its count is B - off)
        if (i == f.nParts - 1) snprintf(b, sizeof(b), " | %d+rest ", f.parts[i].off);
        else snprintf(b, sizeof(b), " | %d+%d ", f.parts[i].off, f.parts[i].count);
        s += b + planText(f.parts[i].plan) + " " + precName(f.parts[i].trunkPrec);
    }
    return s;
}

// the form of every B of 1 .. 4 cus + 64 ([0] unused)
std::vector<std::string> formsOf(const LaunchConfig& c) {
    std::vector<std::string> f(4 * c.cus + 65);
    for (int B = 1; B < (int)f.size(); ++B) f[B] = formText(chooseLaunchForm(c, B), B, c.prec);
    return f;
}

// runs of equal forms on one line each; with `first`, only the batch sizes whose form differs from first's
std::string tableOf(const std::vector<std::string>& f, const std::vector<std::string>* first) {
    std::string out;
    for (int B = 1, lo = 0; B <= (int)f.size(); ++B) {
        const bool shown = B < (int)f.size() && !(first && f[B] == (*first)[B]);
        if (lo && !(shown && f[B] == f[lo])) {
            out += std::to_string(lo) + ".." + std::to_string(B - 1) + " " + f[lo] + "\n";
            lo = 0;
        }
        if (shown && !lo) lo = B;
    }
    return out;
}

typedef std::function<void(LaunchConfig&)> Knob;

// each knob at the values its tests and the evaluator's checks admit, away from its default
std::vector<std::pair<std::string, Knob>> knobs() {
    std::vector<std::pair<std::string, Knob>> k;
#define KNOB(field, value) k.push_back({#field "=" #value, [](LaunchConfig& c) { c.field = value; }})
    KNOB(useTrunkKernel, 0); KNOB(useTrunkKernel, 1);
    KNOB(coopForced, 1);
    KNOB(coopSameXcd, false);
    KNOB(chainMinBatch, 64);
    KNOB(chainDelayUs, -1); KNOB(chainDelayUs, 50);
    KNOB(numChains, 1); KNOB(numChains, 3); KNOB(numChains, 4);
    KNOB(teamMaxBatch, 0); KNOB(teamMaxBatch, 8);
    KNOB(teamForceRowGroups, 1); KNOB(teamForceRowGroups, 2); KNOB(teamForceRowGroups, 3);
    KNOB(ksplit4Max, 0); KNOB(ksplit4Max, 32);
    KNOB(tuning.nb, 1); KNOB(tuning.nb, 2);
    KNOB(tuning.nwaves, 1); KNOB(tuning.nwaves, 2); KNOB(tuning.nwaves, 4);
    KNOB(tuning.nfrag, 1); KNOB(tuning.nfrag, 2); KNOB(tuning.nfrag, 4);
    KNOB(tuning.msplit, 1); KNOB(tuning.msplit, 2);
    KNOB(tuning.splitBatch, 0);
    KNOB(tuning.splitBatchMax3, 8); KNOB(tuning.splitBatchMax3, 12);
    KNOB(tuning.rowsplit8Max, 0); KNOB(tuning.rowsplit8Max, 16);
    KNOB(tuning.ksplit3, 0);
    KNOB(tuning.slabSplit, 1);
    KNOB(tuning.fullTilesOnly, true);
#undef KNOB
    // (64 blocks: more 3x3 layers than a cooperative launch has flag values for)
    k.push_back({"blocks=64", [](LaunchConfig& c) { c.blocks = 64; c.trunkLayerCount = 129; }});
    return k;
}

} // namespace

// The grid: fn(section, variant, config) for every configuration, section by section.
void forEachGridConfig(const std::function<void(const std::string&, const std::string&, const LaunchConfig&)>& fn) {
    static const int kShapes[][2] = {{128, 128}, {192, 128}, {192, 192}, {256, 128}, {256, 256}, {384, 128}};
    for (int cus : {256, 64, 32}) // (128 left out: the table's size)
        for (int prec = kFp32; prec <= kF16m6; ++prec)
            for (const auto& shape : kShapes) {
                LaunchConfig base; // a 20-block net
                base.cus = cus; base.prec = prec; base.F = shape[0]; base.cpad = shape[1];
                base.blocks = 20; base.trunkLayerCount = 41;
                char section[96];
                snprintf(section, sizeof(section), "cus=%d prec=%s F=%d cpad=%d", cus, kPrecNames[prec], shape[0], shape[1]);
                for (int v = 7; v >= 0; --v) {
                    LaunchConfig c = base;
                    c.teamAvailable = v & 4; c.coopAvailable = v & 2; c.outsideM8Window = !(v & 1);
                    char variant[64];
                    snprintf(variant, sizeof(variant), "team=%d coop=%d outside=%d", (int)c.teamAvailable, (int)c.coopAvailable,
                             (int)c.outsideM8Window);
                    fn(section, variant, c);
                }
                if (cus == 32) continue; // (the knobs at 256 and 64 CUs only: the table's size)
                for (const auto& k : knobs()) {
                    LaunchConfig c = base;
                    c.teamAvailable = c.coopAvailable = true;
                    k.second(c);
                    fn(section, k.first, c);
                }
            }
}

#ifndef FORM_DUMP_NO_MAIN
int main() {
    std::string section, body;
    std::vector<std::string> first;                          // the forms of the section's first variant
    std::vector<std::string> order;                          // the other variants' differences, in order of appearance
    std::map<std::string, std::string> sharers;              // differences -> the variants that have them
    std::map<std::string, std::string> seen;                 // a section's text -> the first section that had it
    std::map<std::string, std::string> blocks;               // a variant's lines -> where they were first printed
    auto flush = [&] {
        if (section.empty()) return;
        for (const std::string& d : order) {
            // (a longer run of lines that an earlier section printed under a variant is named, not repeated)
            const bool again = blocks.count(d) && d.size() > 200;
            body += "-- " + sharers[d] + (again ? ": the lines of " + blocks[d] + "\n" : "\n" + d);
            if (!blocks.count(d)) blocks[d] = "[" + section + " -- " + sharers[d].substr(0, sharers[d].find(',')) + "]";
        }
        if (seen.count(body)) printf("== %s: same as %s\n", section.c_str(), seen[body].c_str());
        else { printf("== %s\n%s", section.c_str(), body.c_str()); seen[body] = section; }
        order.clear();
        sharers.clear();
    };
    forEachGridConfig([&](const std::string& s, const std::string& variant, const LaunchConfig& c) {
        if (s != section) {
            flush();
            section = s;
            first = formsOf(c);
            body = tableOf(first, nullptr);
            return;
        }
        const std::string d = tableOf(formsOf(c), &first);
        if (!sharers.count(d)) { order.push_back(d); sharers[d] = variant; }
        else sharers[d] += ", " + variant;
    });
    flush();
    return 0;
}
#endif
