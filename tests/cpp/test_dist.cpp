// The distance family through the C++ facade on the GPU: the reference's goldens
// (tests/integration.rs:63-67, 76-80) and doctests (src/analysis/seq.rs:64-73, 143-151) of
// hamming_distance and transition_transversion_ratio, and a 3 x 3 p_distance_matrix
// (src/analysis/stat.rs:138-152).
#include <cmath>
#include <cstdio>

#include "biogarden.hpp"

using namespace biogarden;

int main(int argc, char** argv) {
  const std::string fix = argc > 1 ? argv[1] : "tests/golden/reference_fixtures";
  int fails = 0;
  {
    auto in = io::fasta::read_tile(fix + "/input/hamming_distance.fasta");
    const size_t h = analysis::seq::hamming_distance(in[0], in[1]).unwrap();
    const size_t d = analysis::seq::hamming_distance(ds::Sequence("GAGCCTACTAACGGGAT"),
                                                     ds::Sequence("CATCGTAATGACGGCCT")).unwrap();
    std::printf("hamming_distance %zu (expect 477), doctest %zu (expect 7)\n", h, d);
    fails += (h != 477) + (d != 7);
    auto e = analysis::seq::hamming_distance(ds::Sequence("ACGT"), ds::Sequence("ACG"));
    fails += !(e.is_err() && e.error() == BioError::InvalidInputSize);
  }
  {
    auto in = io::fasta::read_tile(fix + "/input/transversions.fasta");
    const double r = analysis::seq::transition_transversion_ratio(in[0], in[1]).unwrap();
    const double d = analysis::seq::transition_transversion_ratio(
        ds::Sequence("TTAGGGACTGGATTATTTCGTGATCGTTGTAGTTATTGGAAGTACGGGCATCAACCCAGTT"),
        ds::Sequence("TCAACGGCTGGATAATTTCGCGATCGTGCTGGTTACTGGCGGTACGAGTGTTCCTTTGGGT")).unwrap();
    std::printf("ts/tv %.17g (expect 2.032258064516129), doctest %.17g (expect 1.875)\n", r, d);
    fails += (r != 2.032258064516129) + (d != 1.875);
    auto e = analysis::seq::transition_transversion_ratio(ds::Sequence("A"), ds::Sequence(""));
    fails += !(e.is_err() && e.error() == BioError::InvalidInputSize);
    // every mismatch a transition: t / 0.0 = inf; no mismatch: 0.0 / 0.0 = NaN (seq.rs:173)
    fails += !std::isinf(analysis::seq::transition_transversion_ratio(ds::Sequence("CA"), ds::Sequence("TG")).unwrap());
    fails += !std::isnan(analysis::seq::transition_transversion_ratio(ds::Sequence("CA"), ds::Sequence("CA")).unwrap());
  }
  {
    ds::Tile t;
    t.push(ds::Sequence("ACGTACGT"));
    t.push(ds::Sequence("ACGTTCGA"));
    t.push(ds::Sequence("TCGTACGA"));
    const auto m = analysis::stat::p_distance_matrix(t);
    const float want[9] = {0.f, 2.f / 8.f, 2.f / 8.f, 2.f / 8.f, 0.f, 2.f / 8.f, 2.f / 8.f, 2.f / 8.f, 0.f};
    bool ok = m.rows == 3 && m.values.size() == 9;
    for (size_t k = 0; ok && k < 9; ++k) ok = m.values[k] == want[k];
    std::printf("p_distance_matrix %s\n", ok ? "ok" : "MISMATCH");
    fails += !ok;
    bool panicked = false;
    try { analysis::stat::p_distance_matrix(ds::Tile()); } catch (const ReferencePanic&) { panicked = true; }
    fails += !panicked;
  }
  std::printf("%s\n", fails ? "FAILED" : "dist ok");
  return fails ? 1 : 0;
}
