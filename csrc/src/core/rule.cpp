// gol-mi355x: rule strings (see rule.hpp).
#include "gol/rule.hpp"

#include <cctype>

namespace gol {

namespace {

const char* kB0Text =
    "B0 rules are out of scope: the dead background would come alive, and the engine's zeroed slack rows, trash "
    "lanes and masked tail bits assume dead stays dead";

[[noreturn]] void bad(const std::string& s, const std::string& why) {
    throw Error("invalid rule '" + s + "': " + why);
}

}  // namespace

Rule Rule::from_masks(unsigned birth, unsigned survive) {
    const std::string name = strprintf("(birth 0x%x, survive 0x%x)", birth, survive);
    if (birth > 0x1FFu || survive > 0x1FFu) bad(name, "neighbour counts run from 0 to 8");
    if (birth & 1u) bad(name, kB0Text);
    Rule r;
    r.birth = (u16)birth;
    r.survive = (u16)survive;
    return r;
}

Rule Rule::parse(const std::string& s) {
    std::string low;
    for (char c : s) low += (char)std::tolower((unsigned char)c);
    static const struct {
        const char* name;
        const char* rule;
    } aliases[] = {{"conway", "b3/s23"},         {"life", "b3/s23"}, {"highlife", "b36/s23"},
                   {"daynight", "b3678/s34678"}, {"seeds", "b2/s"},  {"replicator", "b1357/s1357"}};
    for (const auto& a : aliases)
        if (low == a.name) low = a.rule;
    unsigned mask[2] = {0, 0};  // birth, survive
    bool seen[2] = {false, false};
    size_t i = 0;
    for (int part = 0; part < 2; ++part) {
        if (part == 1) {
            if (i >= low.size() || low[i] != '/') bad(s, "expected B<digits>/S<digits>");
            ++i;
        }
        if (i >= low.size() || (low[i] != 'b' && low[i] != 's'))
            bad(s, part == 0 ? "expected B<digits>/S<digits>" : "missing B or S part");
        const int which = low[i] == 'b' ? 0 : 1;
        if (seen[which]) bad(s, which == 0 ? "two B parts, missing S part" : "two S parts, missing B part");
        seen[which] = true;
        ++i;
        for (; i < low.size() && std::isdigit((unsigned char)low[i]); ++i) {
            const int d = low[i] - '0';
            if (d > 8) bad(s, "digit 9: neighbour counts run from 0 to 8");
            if (mask[which] & (1u << d)) bad(s, strprintf("digit %d repeated", d));
            mask[which] |= 1u << d;
        }
    }
    if (i != low.size()) bad(s, "trailing text '" + s.substr(i) + "'");
    if (mask[0] & 1u) bad(s, kB0Text);
    Rule r;
    r.birth = (u16)mask[0];
    r.survive = (u16)mask[1];
    return r;
}

std::string Rule::str() const {
    std::string out = "B";
    for (int d = 0; d <= 8; ++d)
        if (birth & (1u << d)) out += (char)('0' + d);
    out += "/S";
    for (int d = 0; d <= 8; ++d)
        if (survive & (1u << d)) out += (char)('0' + d);
    return out;
}

}  // namespace gol
