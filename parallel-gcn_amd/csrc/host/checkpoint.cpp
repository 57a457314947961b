// parallel-gcn_amd/csrc/host/checkpoint.cpp -- see checkpoint.hpp for the format.
#include "checkpoint.hpp"

#include <cstddef>
#include <cstdio>
#include <cstring>

#include "../common.hpp"
#include "data.hpp"

namespace pgcn {

namespace {
constexpr char kCkMagic[8] = {'P', 'G', 'C', 'N', 'C', 'K', '0', '1'};

struct CkHeader {
  char magic[8];
  uint32_t version, n_layers;
  int64_t num_nodes;
  int32_t dims[18];
  float dropouts[16];
  uint32_t seed, flags;
  int64_t adam_steps, draw_epochs, epochs, n_results, n_weights;
  uint64_t checksum;
};
static_assert(sizeof(CkHeader) == 216, "checkpoint header layout");

// version 5: between the header and the payload
struct CkHeadsExt {
  uint32_t heads;
  float attention_dropout;
  uint64_t zero;
};
static_assert(sizeof(CkHeadsExt) == 16, "checkpoint extension layout");

CkHeadsExt heads_ext(const Checkpoint &ck) {
  return CkHeadsExt{(uint32_t)ck.heads, ck.attention_dropout, 0};
}

// version 6: in the same place
struct CkSageExt {
  uint32_t aggregator, root_weight;
  uint64_t zero;
};
static_assert(sizeof(CkSageExt) == 16, "checkpoint extension layout");

CkSageExt sage_ext(const Checkpoint &ck) {
  return CkSageExt{(uint32_t)ck.aggregator, (uint32_t)ck.root_weight, 0};
}

// version 7: behind the other two blocks
struct CkReadoutExt {
  uint32_t readout, num_graphs;
  uint64_t zero;
};
static_assert(sizeof(CkReadoutExt) == 16, "checkpoint extension layout");

CkReadoutExt readout_ext(const Checkpoint &ck) {
  return CkReadoutExt{(uint32_t)ck.readout, (uint32_t)ck.num_graphs, 0};
}

// version 8: behind version 7's three blocks
struct CkLinksExt {
  uint32_t link_decoder, zero;
  uint64_t num_pairs;
};
static_assert(sizeof(CkLinksExt) == 16, "checkpoint extension layout");

CkLinksExt links_ext(const Checkpoint &ck) {
  return CkLinksExt{(uint32_t)ck.link_decoder, 0, (uint64_t)ck.num_pairs};
}

// versions 7 and 8 carry the heads, SAGE and readout blocks whatever the layer family
bool three_blocks(uint32_t version) {
  return version == (uint32_t)kCheckpointVersionReadout ||
         version == (uint32_t)kCheckpointVersionLinks;
}

uint64_t ck_hash(const CkHeader &h, const Checkpoint &ck) {
  uint64_t x = fnv1a(kFnvBasis, &h, offsetof(CkHeader, checksum));
  if (three_blocks(h.version)) {
    const CkHeadsExt e = heads_ext(ck);
    const CkSageExt se = sage_ext(ck);
    const CkReadoutExt re = readout_ext(ck);
    x = fnv1a(x, &e, sizeof e);
    x = fnv1a(x, &se, sizeof se);
    x = fnv1a(x, &re, sizeof re);
  }
  if (h.version == (uint32_t)kCheckpointVersionLinks) {
    const CkLinksExt le = links_ext(ck);
    x = fnv1a(x, &le, sizeof le);
  }
  if (h.version == (uint32_t)kCheckpointVersionHeads) {
    const CkHeadsExt e = heads_ext(ck);
    x = fnv1a(x, &e, sizeof e);
  }
  if (h.version == (uint32_t)kCheckpointVersionSage) {
    const CkSageExt e = sage_ext(ck);
    x = fnv1a(x, &e, sizeof e);
  }
  for (const auto *vec : {&ck.results, &ck.w, &ck.m, &ck.v})
    x = fnv1a(x, vec->data(), vec->size() * sizeof(float));
  return x;
}

bool write_floats(std::FILE *f, const std::vector<float> &v) {
  return v.empty() || std::fwrite(v.data(), sizeof(float), v.size(), f) == v.size();
}

bool read_floats(std::FILE *f, std::vector<float> &v, long long n) {
  v.resize((size_t)n);
  return n == 0 || std::fread(v.data(), sizeof(float), (size_t)n, f) == (size_t)n;
}

long long weight_count(const int32_t *dims, int n_layers, int root_weight = 0) {
  long long n = 0;
  for (int l = 0; l < n_layers; l++) n += (long long)dims[l] * dims[l + 1] * (root_weight ? 2 : 1);
  return n;
}

long long norm_count_of(const int32_t *dims, int n_layers) {
  long long n = 0;
  for (int l = 1; l < n_layers; l++) n += 2LL * dims[l];
  return n;
}

long long attn_count_of(const int32_t *dims, int n_layers) {
  long long n = 0;
  for (int l = 1; l <= n_layers; l++) n += 2LL * dims[l];
  return n;
}

// whether a file of this version may carry these flag bits (false: unknown version or bit)
bool version_flags_ok(uint32_t version, uint32_t flags) {
  if (version == (uint32_t)kCheckpointVersion) return (flags & ~kCheckpointKnownFlags) == 0;
  if (version == (uint32_t)kCheckpointVersionLayerNorm)
    return (flags & kCheckpointLayerNorm) &&
           (flags & ~(kCheckpointResidual | kCheckpointLayerNorm)) == 0;
  if (version == (uint32_t)kCheckpointVersionLayerNormMultilabel)
    return (flags & kCheckpointLayerNorm) && (flags & kCheckpointMultilabel) &&
           (flags & ~(kCheckpointKnownFlags | kCheckpointLayerNorm)) == 0;
  if (version == (uint32_t)kCheckpointVersionAttention ||
      version == (uint32_t)kCheckpointVersionHeads)
    return (flags & kCheckpointAttention) &&
           (flags & ~(kCheckpointKnownFlags | kCheckpointLayerNorm | kCheckpointAttention)) == 0;
  if (version == (uint32_t)kCheckpointVersionSage)
    return (flags & kCheckpointSage) &&
           (flags & ~(kCheckpointKnownFlags | kCheckpointLayerNorm | kCheckpointSage)) == 0;
  if (version == (uint32_t)kCheckpointVersionReadout)  // (the engine never has bits 2, or 3 with 4)
    return (flags & kCheckpointReadout) && !(flags & kCheckpointMultilabel) &&
           !((flags & kCheckpointAttention) && (flags & kCheckpointSage)) &&
           (flags & ~(kCheckpointResidual | kCheckpointLayerNorm | kCheckpointAttention |
                      kCheckpointSage | kCheckpointReadout)) == 0;
  if (version == (uint32_t)kCheckpointVersionLinks)  // (never bits 2 or 5, or 3 with 4)
    return (flags & kCheckpointLinks) &&
           !((flags & kCheckpointAttention) && (flags & kCheckpointSage)) &&
           (flags & ~(kCheckpointResidual | kCheckpointLayerNorm | kCheckpointAttention |
                      kCheckpointSage | kCheckpointLinks)) == 0;
  return false;
}

long long expected_weights(const int32_t *dims, int n_layers, uint32_t flags,
                           int root_weight = 0) {
  return weight_count(dims, n_layers, root_weight) +
         ((flags & kCheckpointLayerNorm) ? norm_count_of(dims, n_layers) : 0) +
         ((flags & kCheckpointAttention) ? attn_count_of(dims, n_layers) : 0);
}

// the extension's values against the file's version and hidden dims (the engine's own rules)
bool heads_ok(uint32_t version, uint32_t flags, const int32_t *dims, int n_layers,
              long long heads, float p) {
  const bool v7 = three_blocks(version) && (flags & kCheckpointAttention);
  if (version != (uint32_t)kCheckpointVersionHeads && !v7) return heads == 1 && p == 0.0f;
  if (heads < 1 || heads > 32 || !(p >= 0.0f && p < 1.0f) || (!v7 && heads == 1 && p == 0.0f))
    return false;
  for (int l = 1; heads > 1 && l < n_layers; l++) {
    const long long dh = dims[l] / heads;
    if (dims[l] % heads != 0 || dh < 4 || dh > 128 || (dh & (dh - 1)) != 0) return false;
  }
  return true;
}

// version 6's block against the file's version (the engine's own rules)
bool sage_ok(uint32_t version, uint32_t flags, const int32_t *dims, int n_layers,
             long long aggregator, long long root_weight) {
  const bool v7 = three_blocks(version) && (flags & kCheckpointSage);
  if (version != (uint32_t)kCheckpointVersionSage && !v7)
    return aggregator == 0 && root_weight == 0;
  if (aggregator < 1 || aggregator > 2 || root_weight < 0 || root_weight > 1) return false;
  for (int l = 1; l <= n_layers; l++)
    if (dims[l] > 128) return false;
  return true;
}
// version 7's own block against the file's version
bool readout_ok(uint32_t version, long long readout, long long num_graphs, long long num_nodes) {
  if (version != (uint32_t)kCheckpointVersionReadout) return readout == 0 && num_graphs == 0;
  return readout >= 1 && readout <= 3 && num_graphs >= 1 && num_graphs < (1LL << 31) &&
         num_nodes >= 0;
}
// version 8's own block against the file's version
bool links_ok(uint32_t version, long long decoder, long long num_pairs) {
  if (version != (uint32_t)kCheckpointVersionLinks) return decoder == 0 && num_pairs == 0;
  return decoder == 1 && num_pairs >= 1 && num_pairs < (1LL << 31);
}
}  // namespace


void write_checkpoint(const std::string &path, const Checkpoint &ck) {
  const int L = ck.n_layers;
  PGCN_CHECK(L >= 2 && L <= PGCN_MAX_LAYERS && (int)ck.dims.size() == L + 1 &&
                 (int)ck.dropouts.size() == L && ck.results.size() % 4 == 0 &&
                 ck.results.size() / 4 <= (size_t)kCheckpointMaxResults &&
                 ck.m.size() == ck.w.size() && ck.v.size() == ck.w.size(),
             PGCN_E_INVALID, "checkpoint: inconsistent state");
  CkHeader h{};
  std::memcpy(h.magic, kCkMagic, 8);
  h.version = (uint32_t)ck.version;
  h.n_layers = (uint32_t)L;
  h.num_nodes = ck.num_nodes;
  for (int l = 0; l <= L; l++) h.dims[l] = ck.dims[(size_t)l];
  for (int l = 0; l < L; l++) h.dropouts[l] = ck.dropouts[(size_t)l];
  h.seed = ck.seed;
  h.flags = ck.flags;
  PGCN_CHECK(version_flags_ok(h.version, ck.flags), PGCN_E_INVALID,
             "checkpoint: flags unknown to the file's version");
  h.adam_steps = ck.adam_steps;
  h.draw_epochs = ck.draw_epochs;
  h.epochs = ck.epochs;
  h.n_results = (int64_t)(ck.results.size() / 4);
  h.n_weights = (int64_t)ck.w.size();
  PGCN_CHECK(readout_ok(h.version, ck.readout, ck.num_graphs, ck.num_nodes), PGCN_E_INVALID,
             "checkpoint: readout / graph count do not match the file's version");
  PGCN_CHECK(links_ok(h.version, ck.link_decoder, ck.num_pairs), PGCN_E_INVALID,
             "checkpoint: link decoder / pair count do not match the file's version");
  PGCN_CHECK(sage_ok(h.version, h.flags, h.dims, L, ck.aggregator, ck.root_weight), PGCN_E_INVALID,
             "checkpoint: aggregator / root weight do not match the file's version");
  PGCN_CHECK(h.n_weights == expected_weights(h.dims, L, h.flags, ck.root_weight), PGCN_E_INVALID,
             "checkpoint: weight count does not match the layer dims");
  PGCN_CHECK(heads_ok(h.version, h.flags, h.dims, L, ck.heads, ck.attention_dropout),
             PGCN_E_INVALID,
             "checkpoint: heads / attention dropout do not match the file's version");
  const CkHeadsExt ext = heads_ext(ck);
  const bool v7 = three_blocks(h.version);
  const bool v8 = h.version == (uint32_t)kCheckpointVersionLinks;
  const bool with_ext = h.version == (uint32_t)kCheckpointVersionHeads || v7;
  const CkSageExt sext = sage_ext(ck);
  const bool with_sage = h.version == (uint32_t)kCheckpointVersionSage || v7;
  const CkReadoutExt rext = readout_ext(ck);
  const CkLinksExt lext = links_ext(ck);
  h.checksum = ck_hash(h, ck);
  const std::string tmp = path + ".tmp";
  std::FILE *f = std::fopen(tmp.c_str(), "wb");
  if (!f) throw Error(PGCN_E_IO, "checkpoint: cannot write " + tmp);
  bool ok = std::fwrite(&h, sizeof(h), 1, f) == 1 &&
            (!with_ext || std::fwrite(&ext, sizeof(ext), 1, f) == 1) &&
            (!with_sage || std::fwrite(&sext, sizeof(sext), 1, f) == 1) &&
            (!v7 || std::fwrite(&rext, sizeof(rext), 1, f) == 1) &&
            (!v8 || std::fwrite(&lext, sizeof(lext), 1, f) == 1) &&
            write_floats(f, ck.results) &&
            write_floats(f, ck.w) && write_floats(f, ck.m) && write_floats(f, ck.v);
  ok = (std::fclose(f) == 0) && ok;
  if (ok) ok = std::rename(tmp.c_str(), path.c_str()) == 0;  // readers never see a partial file
  if (!ok) {
    std::remove(tmp.c_str());
    throw Error(PGCN_E_IO, "checkpoint: cannot write " + path);
  }
}

Checkpoint read_checkpoint(const std::string &path) {
  std::FILE *f = std::fopen(path.c_str(), "rb");
  if (!f) throw Error(PGCN_E_IO, "checkpoint: cannot open " + path);
  CkHeader h{};
  Checkpoint ck;
  bool ok = std::fread(&h, sizeof(h), 1, f) == 1 && std::memcmp(h.magic, kCkMagic, 8) == 0 &&
            version_flags_ok(h.version, h.flags) && h.n_layers >= 2 &&
            h.n_layers <= PGCN_MAX_LAYERS && h.num_nodes > 0;
  const int L = ok ? (int)h.n_layers : 0;
  for (int l = 0; ok && l <= L; l++) ok = h.dims[l] > 0 && h.dims[l] <= (1 << 24);
  ok = ok && h.adam_steps >= 0 && h.draw_epochs >= 0 && h.epochs >= 0 && h.n_results >= 0 &&
       h.n_results <= kCheckpointMaxResults && h.n_results <= h.epochs &&
       h.n_weights < (1LL << 31);
  const bool v7 = ok && three_blocks(h.version);
  if (ok && (h.version == (uint32_t)kCheckpointVersionHeads || v7)) {
    CkHeadsExt e{};
    ok = std::fread(&e, sizeof(e), 1, f) == 1 && e.zero == 0 && e.heads <= 32;
    ck.heads = (int)e.heads;
    ck.attention_dropout = e.attention_dropout;
  }
  if (ok && (h.version == (uint32_t)kCheckpointVersionSage || v7)) {
    CkSageExt e{};
    ok = std::fread(&e, sizeof(e), 1, f) == 1 && e.zero == 0 && e.aggregator <= 2 &&
         e.root_weight <= 1;
    ck.aggregator = (int)e.aggregator;
    ck.root_weight = (int)e.root_weight;
  }
  if (ok && v7) {
    CkReadoutExt e{};
    ok = std::fread(&e, sizeof(e), 1, f) == 1 && e.zero == 0 && e.readout <= 3 &&
         e.num_graphs < (1u << 31);
    ck.readout = (int)e.readout;
    ck.num_graphs = (int)e.num_graphs;
  }
  if (ok && h.version == (uint32_t)kCheckpointVersionLinks) {
    CkLinksExt e{};
    ok = std::fread(&e, sizeof(e), 1, f) == 1 && e.zero == 0 && e.link_decoder <= 1 &&
         e.num_pairs < (1ull << 31);
    ck.link_decoder = (int)e.link_decoder;
    ck.num_pairs = (long long)e.num_pairs;
  }
  ok = ok && links_ok(h.version, ck.link_decoder, ck.num_pairs) && heads_ok(h.version, h.flags, h.dims, L, ck.heads, ck.attention_dropout) &&
       sage_ok(h.version, h.flags, h.dims, L, ck.aggregator, ck.root_weight) &&
       readout_ok(h.version, ck.readout, ck.num_graphs, h.num_nodes) &&
       h.n_weights == expected_weights(h.dims, L, h.flags, ck.root_weight);
  ok = ok && read_floats(f, ck.results, h.n_results * 4) && read_floats(f, ck.w, h.n_weights) &&
       read_floats(f, ck.m, h.n_weights) && read_floats(f, ck.v, h.n_weights);
  ok = ok && std::fgetc(f) == EOF;  // nothing trailing
  std::fclose(f);
  if (!ok || ck_hash(h, ck) != h.checksum)
    throw Error(PGCN_E_IO, "checkpoint: not a valid checkpoint (truncated, corrupted or another "
                           "version): " + path);
  ck.version = (int)h.version;
  ck.n_layers = L;
  ck.num_nodes = h.num_nodes;
  ck.dims.assign(h.dims, h.dims + L + 1);
  ck.dropouts.assign(h.dropouts, h.dropouts + L);
  ck.seed = h.seed;
  ck.flags = h.flags;
  ck.adam_steps = h.adam_steps;
  ck.draw_epochs = h.draw_epochs;
  ck.epochs = h.epochs;
  return ck;
}

}  // namespace pgcn
