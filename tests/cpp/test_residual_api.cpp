// tests/cpp/test_residual_api.cpp -- the reference-shaped C++ API's ResidualConnection
// (include/pgcn.hpp; reference include/module.cuh:149-161).
//
//   test_residual_api <root> <name> <epochs>
//     assembles a 4-layer GCN with hidden widths (16,16,16) from Variable / Module objects, in
//     the module order of hpdga-spring23's GCN constructor (src/gcn.cpp:64-128) extended to
//     L layers, with a ResidualConnection(prev = the layer's input, current = its output) after
//     the ReLU of each of the two middle layers, and runs train_epoch / eval(2) with every
//     module's backward called in reverse order.  Dropout 0.5 everywhere, Adam over
//     {W1 decayed, W2, W3, W4}.
//   test_residual_api mismatch <root> <name>
//     a ResidualConnection over variables of different widths must throw; prints "mismatch ok".
// Prints one line per epoch: "epoch=<e> <train_loss> <train_acc> <val_loss> <val_acc>" (%.9g);
// tests/test_gpu_residual_api.py compares them with the engine's residual model.
#include <pgcn.hpp>

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <memory>
#include <string>
#include <vector>

using namespace pgcn::api;

static std::vector<integer> truth_of(const GCNData &d, natural split) {
  std::vector<integer> t(d.label.size());
  for (size_t i = 0; i < t.size(); i++) t[i] = d.split[i] == split ? d.label[i] : -1;
  return t;
}

static int run(int argc, char **argv);

int main(int argc, char **argv) {
  try {
    return run(argc, argv);
  } catch (const std::exception &e) {
    fprintf(stderr, "test_residual_api: %s\n", e.what());
    return 1;
  }
}

static int run(int argc, char **argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s <root> <name> <epochs> | mismatch <root> <name>\n", argv[0]);
    return 2;
  }
  const bool mismatch = std::string(argv[1]) == "mismatch";
  GCNParams params;
  GCNData data;
  Parser parser(&params, &data, mismatch ? argv[3] : argv[2], mismatch ? argv[2] : argv[1]);
  if (!parser.parse()) {
    fprintf(stderr, "cannot read the dataset\n");
    return 1;
  }
  const int epochs = mismatch ? 0 : atoi(argv[3]);
  AdamParams adam;  // lr 0.01, weight decay 5e-4 (hpdga defaults)
  const natural N = params.num_nodes, F = params.input_dim, H = 16, C = params.output_dim;
  const real p = 0.5f;

  Variable::initialize_random();
  smart_stream stream;
  DevSparseIndex feat_index(data.feature_index), graph(data.graph);
  integer *dev_truth = nullptr;
  (void)hipMalloc(&dev_truth, sizeof(integer) * N);
  real *dev_graph_value = nullptr;
  (void)hipMalloc(&dev_graph_value, sizeof(real) * data.graph_value.size());
  (void)hipMemcpy(dev_graph_value, data.graph_value.data(),
                  sizeof(real) * data.graph_value.size(), hipMemcpyHostToDevice);
  real loss = 0.0f;

  if (mismatch) {
    auto a1 = std::make_shared<Variable>(N * H), a2 = std::make_shared<Variable>(N * H);
    auto b1 = std::make_shared<Variable>(N * 8), b2 = std::make_shared<Variable>(N * 8);
    GraphSum ga(a1, a2, &graph, dev_graph_value, H);
    GraphSum gb(b1, b2, &graph, dev_graph_value, 8);
    bool thrown = false;
    try {
      ResidualConnection bad(a2, b2);
    } catch (const std::exception &) {
      thrown = true;
    }
    (void)hipFree(dev_truth);
    (void)hipFree(dev_graph_value);
    printf("mismatch %s\n", thrown ? "ok" : "BAD");
    return thrown ? 0 : 1;
  }

  // weights first, in layer order (the engine's glorot order)
  auto W1 = std::make_shared<Variable>(F * H, true, true, F, H);
  auto W2 = std::make_shared<Variable>(H * H, true, true, H, H);
  auto W3 = std::make_shared<Variable>(H * H, true, true, H, H);
  auto W4 = std::make_shared<Variable>(H * C, true, true, H, C);
  for (auto &w : {W1, W2, W3, W4}) w->glorot();

  std::vector<std::unique_ptr<Module>> modules;
  auto input = std::make_shared<Variable>((natural)data.feature_index.indices.size(), false);
  input->from_host(data.feature_value);
  modules.push_back(std::make_unique<Dropout>(input, p));
  auto var1 = std::make_shared<Variable>(N * H);
  modules.push_back(std::make_unique<SparseMatmul>(input, W1, var1, &feat_index, N, F, H));
  auto h = std::make_shared<Variable>(N * H);
  modules.push_back(std::make_unique<GraphSum>(var1, h, &graph, dev_graph_value, H));
  modules.push_back(std::make_unique<ReLU>(h));
  for (const auto &W : {W2, W3}) {  // the two residual layers
    modules.push_back(std::make_unique<Dropout>(h, p));
    auto v1 = std::make_shared<Variable>(N * H);
    modules.push_back(std::make_unique<Matmul>(h, W, v1, N, H, H));
    auto v2 = std::make_shared<Variable>(N * H);
    modules.push_back(std::make_unique<GraphSum>(v1, v2, &graph, dev_graph_value, H));
    modules.push_back(std::make_unique<ReLU>(v2));
    modules.push_back(std::make_unique<ResidualConnection>(h, v2));
    h = v2;
  }
  modules.push_back(std::make_unique<Dropout>(h, p));
  auto o1 = std::make_shared<Variable>(N * C);
  modules.push_back(std::make_unique<Matmul>(h, W4, o1, N, H, C));
  auto output = std::make_shared<Variable>(N * C);
  modules.push_back(std::make_unique<GraphSum>(o1, output, &graph, dev_graph_value, C));
  auto ce = std::make_unique<CrossEntropyLoss>(output, dev_truth, &loss, C);
  CrossEntropyLoss *cep = ce.get();
  modules.push_back(std::move(ce));
  Adam optimizer(std::vector<shared_ptr<Variable>>{W1, W2, W3, W4},
                 std::vector<bool>{true, false, false, false}, &adam);

  auto l2_penalty = [&]() {  // hpdga gcn.cpp:166-173 (float, element order)
    const std::vector<real> w = W1->to_host();
    float l2 = 0.0f;
    for (float x : w) l2 += x * x;
    return adam.weight_decay * l2 / 2;
  };
  auto pass = [&](natural split, bool training) {
    const std::vector<integer> t = truth_of(data, split);
    stream.sync();
    (void)hipMemcpy(dev_truth, t.data(), sizeof(integer) * N, hipMemcpyHostToDevice);
    natural labelled = 0;
    for (integer x : t) labelled += x >= 0;
    cep->set_num_samples(labelled);
    for (auto &m : modules) m->forward(training, stream);
    stream.sync();
    const float l = loss + l2_penalty(), acc = cep->accuracy();
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
  (void)hipFree(dev_graph_value);
  return 0;
}
