function [perm,pf,cost,rounds] = assignGoals(po,goals,prm,epsilon,max_rounds)
% Goal assignment ahead of a transition (no reference counterpart: randomTest.m / randomExchange.m hand out labelled goals).
% po, goals: 3 x N (or 1 x 3 x N as randomTest returns them); prm: a dmpc_params_struct (its c sets the metric E1 = diag(1,1,1/c)).
% perm (1 x N, 1-based): agent i flies to goals(:,perm(i)) = pf(:,i), the labelling that minimises the sum of |E1 (po_i - pf_i)|^2 to
% within N*epsilon (default 1e-4 / N); cost: that sum; rounds: auction rounds (-1: the cap max_rounds was met, perm is then all zeros).
po = reshape(po,3,[]); goals = reshape(goals,3,[]);
if nargin < 4, epsilon = []; end
if nargin < 5, max_rounds = 0; end
[perm,pf,cost,rounds] = dmpc_mex('assign', prm, po, goals, epsilon, max_rounds);
end
