// The named fp32 tensors a model handle expects in a state dict, and the strict check of a caller's
// state dict against them (lg_/sg_/sp_/sp_aliked_load_weights).  Host only: no HIP headers.
#pragma once

#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace lg {

struct WeightSchema {
  // registration order is kept: it is the order of <family>_weight_name(h, i)
  void add(std::string name, int64_t numel) {
    index_[name] = (int)names_.size();
    names_.push_back(std::move(name));
    numels_.push_back(numel);
  }
  int size() const { return (int)names_.size(); }
  const std::string& name(int k) const { return names_[k]; }
  int64_t numel(int k) const { return numels_[k]; }
  // -1 when absent
  int find(const std::string& name) const {
    auto it = index_.find(name);
    return it == index_.end() ? -1 : it->second;
  }
  // Strict match of a caller's state dict: every key known, none twice, every size right, none
  // missing.  On success src[k] is the position in the caller's arrays of schema tensor k.
  bool match(int n, const char* const* names, const float* const* tensors, const int64_t* numels, std::vector<int>& src,
             std::string& err) const {
    auto bad = [&err](std::string msg) {
      err = std::move(msg);
      return false;
    };
    src.assign(names_.size(), -1);
    for (int i = 0; i < n; ++i) {
      if (!names[i] || !tensors[i]) return bad("null tensor at index " + std::to_string(i));
      const int k = find(names[i]);
      if (k < 0) return bad(std::string("unexpected key in state_dict: ") + names[i]);
      if (src[k] >= 0) return bad(std::string("duplicate key: ") + names[i]);
      src[k] = i;
      if (numels[i] != numels_[k])
        return bad(std::string("size mismatch for ") + names[i] + ": expected " + std::to_string(numels_[k]) + " got " +
                   std::to_string(numels[i]));
    }
    for (size_t k = 0; k < names_.size(); ++k)
      if (src[k] < 0) return bad("missing key in state_dict: " + names_[k]);
    return true;
  }

 private:
  std::vector<std::string> names_;
  std::vector<int64_t> numels_;
  std::map<std::string, int> index_;
};

}  // namespace lg
