// OakGPU::BuildTrainer (include/oakgpu.hpp): the refusals on the host, then a trainer on the net the test hands over, three rounds of a planted
// gradient block, Adam and the rolling average; the nets, the average and Adam's first moment go to a file that
// tests/test_gpu_build_trainer_cpp.py compares with oak_amd.build.Trainer's.  usage: cpp_build_trainer_smoke NET OUT.  Without a GPU it only links.
#include <cstdio>
#include <cstdlib>
#include <oakgpu.hpp>

static std::vector<uint8_t> slurp(const char *path) {
  std::vector<uint8_t> out;
  if (FILE *f = std::fopen(path, "rb")) {
    uint8_t buf[4096];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + k);
    std::fclose(f);
  }
  return out;
}
template <class T> static void dump(FILE *f, const std::vector<T> &v) { std::fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char **argv) {
  if (oakgpu_device_count() == 0 || argc < 3) { std::puts("no gpu: link check only"); return 0; }
  const std::vector<uint8_t> net = slurp(argv[1]);
  OakGPU::BuildTrainer::check_net(net, 4);
  OakGPU::Context ctx{0};
  OakGPU::BuildTrainer trainer{ctx, net, 4};
  if (trainer.net_bytes() != net || trainer.net_bytes(OAKGPU_BUILD_TRAIN_AVERAGE) != net) return 3;
  const float planted[5] = {0.0f, 1e-3f, -1.0f, 0.5f, -2e-5f};
  std::vector<float> grads(trainer.count());
  for (size_t i = 0; i < grads.size(); ++i) grads[i] = planted[i % 5];
  for (int step = 0; step < 3; ++step) {
    trainer.set_gradients(grads);
    trainer.adam(1e-2f);
    trainer.average(0.9);
  }
  const oakgpu_build_train_report r = trainer.report();
  FILE *f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  dump(f, trainer.net_bytes());
  dump(f, trainer.net_bytes(OAKGPU_BUILD_TRAIN_AVERAGE));
  dump(f, trainer.read(OAKGPU_BUILD_TRAIN_M));
  std::fclose(f);
  std::printf("%zu parameters, policy hidden %u, %llu steps\nok\n", trainer.count(), trainer.layer(0).second, (unsigned long long)r.steps);
  return 0;
}
