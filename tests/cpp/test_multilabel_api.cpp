// tests/cpp/test_multilabel_api.cpp -- the reference-shaped C++ API's BCEWithLogitsLoss
// (include/pgcn.hpp; the reference has no multi-label loss).
//
//   test_multilabel_api <root> <name> <epochs>
//     reads data/<name>.{graph,split,svmlight} with the Parser and the label matrix from
//     data/<name>.labels (line i: the class ids of node i; the class count is the largest id +
//     1), assembles the 2-layer GCN (hidden 16, dropout 0.5) from Variable / Module objects in
//     the module order of hpdga-spring23's GCN constructor (src/gcn.cpp:64-128) ending in
//     BCEWithLogitsLoss instead of CrossEntropyLoss, and runs train_epoch / eval(2).
// Prints one line per epoch: "epoch=<e> <train_loss> <train_acc> <val_loss> <val_acc>" (%.9g);
// tests/test_gpu_multilabel_api.py compares them with the engine's multi-label model.
#include <pgcn.hpp>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

using namespace pgcn::api;

static int run(int argc, char **argv);

int main(int argc, char **argv) {
  try {
    return run(argc, argv);
  } catch (const std::exception &e) {
    fprintf(stderr, "test_multilabel_api: %s\n", e.what());
    return 1;
  }
}

static int run(int argc, char **argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s <root> <name> <epochs>\n", argv[0]);
    return 2;
  }
  GCNParams params;
  GCNData data;
  Parser parser(&params, &data, argv[2], argv[1]);
  if (!parser.parse()) {
    fprintf(stderr, "cannot read the dataset\n");
    return 1;
  }
  const int epochs = atoi(argv[3]);
  const natural N = params.num_nodes, F = params.input_dim, H = 16;
  // the label matrix
  std::vector<std::vector<int>> ids;
  int max_id = -1;
  {
    std::ifstream in(std::string(argv[1]) + "/data/" + argv[2] + ".labels");
    std::string line;
    while (std::getline(in, line)) {
      std::stringstream ss(line);
      ids.emplace_back();
      int j;
      while (ss >> j) {
        ids.back().push_back(j);
        if (j > max_id) max_id = j;
      }
    }
  }
  if (ids.size() != (size_t)N || max_id < 0 || max_id >= 128) {
    fprintf(stderr, "cannot read the labels file\n");
    return 1;
  }
  const natural C = (natural)max_id + 1, words = (C + 31) / 32;
  std::vector<uint32_t> bits((size_t)N * words, 0u);
  for (size_t i = 0; i < ids.size(); i++)
    for (int j : ids[i]) bits[i * words + (size_t)j / 32] |= 1u << (j % 32);

  AdamParams adam;  // lr 0.01, weight decay 5e-4 (hpdga defaults)
  const real p = 0.5f;
  Variable::initialize_random();
  smart_stream stream;
  DevSparseIndex feat_index(data.feature_index), graph(data.graph);
  integer *dev_truth = nullptr;
  (void)hipMalloc(&dev_truth, sizeof(integer) * N);
  uint32_t *dev_bits = nullptr;
  (void)hipMalloc(&dev_bits, sizeof(uint32_t) * bits.size());
  (void)hipMemcpy(dev_bits, bits.data(), sizeof(uint32_t) * bits.size(), hipMemcpyHostToDevice);
  real *dev_graph_value = nullptr;
  (void)hipMalloc(&dev_graph_value, sizeof(real) * data.graph_value.size());
  (void)hipMemcpy(dev_graph_value, data.graph_value.data(),
                  sizeof(real) * data.graph_value.size(), hipMemcpyHostToDevice);
  real loss = 0.0f;

  auto W1 = std::make_shared<Variable>(F * H, true, true, F, H);
  auto W2 = std::make_shared<Variable>(H * C, true, true, H, C);
  W1->glorot();
  W2->glorot();
  std::vector<std::unique_ptr<Module>> modules;
  auto input = std::make_shared<Variable>((natural)data.feature_index.indices.size(), false);
  input->from_host(data.feature_value);
  modules.push_back(std::make_unique<Dropout>(input, p));
  auto var1 = std::make_shared<Variable>(N * H);
  modules.push_back(std::make_unique<SparseMatmul>(input, W1, var1, &feat_index, N, F, H));
  auto h = std::make_shared<Variable>(N * H);
  modules.push_back(std::make_unique<GraphSum>(var1, h, &graph, dev_graph_value, H));
  modules.push_back(std::make_unique<ReLU>(h));
  modules.push_back(std::make_unique<Dropout>(h, p));
  auto o1 = std::make_shared<Variable>(N * C);
  modules.push_back(std::make_unique<Matmul>(h, W2, o1, N, H, C));
  auto output = std::make_shared<Variable>(N * C);
  modules.push_back(std::make_unique<GraphSum>(o1, output, &graph, dev_graph_value, C));
  auto bce = std::make_unique<BCEWithLogitsLoss>(output, dev_truth, dev_bits, words, &loss, C);
  BCEWithLogitsLoss *bcep = bce.get();
  modules.push_back(std::move(bce));
  Adam optimizer(std::vector<shared_ptr<Variable>>{W1, W2}, std::vector<bool>{true, false}, &adam);

  auto l2_penalty = [&]() {  // hpdga gcn.cpp:166-173 (float, element order)
    const std::vector<real> w = W1->to_host();
    float l2 = 0.0f;
    for (float x : w) l2 += x * x;
    return adam.weight_decay * l2 / 2;
  };
  auto pass = [&](natural split, bool training) {
    std::vector<integer> t(data.label.size());
    natural labelled = 0;
    for (size_t i = 0; i < t.size(); i++) {
      t[i] = data.split[i] == (integer)split && data.label[i] >= 0 ? 0 : -1;
      labelled += t[i] >= 0;
    }
    stream.sync();
    (void)hipMemcpy(dev_truth, t.data(), sizeof(integer) * N, hipMemcpyHostToDevice);
    bcep->set_num_samples(labelled);
    for (auto &m : modules) m->forward(training, stream);
    stream.sync();
    const float l = loss + l2_penalty(), acc = bcep->accuracy();
    if (training) {
      for (int i = (int)modules.size() - 1; i >= 0; i--) modules[(size_t)i]->backward(stream);
      optimizer.step(stream);
      stream.sync();
    }
    return std::make_pair(l, acc);
  };
  for (int e = 1; e <= epochs; e++) {
    const auto tr = pass(1, true);
    const auto va = pass(2, false);
    printf("epoch=%d %.9g %.9g %.9g %.9g\n", e, tr.first, tr.second, va.first, va.second);
  }
  (void)hipFree(dev_truth);
  (void)hipFree(dev_bits);
  (void)hipFree(dev_graph_value);
  return 0;
}
