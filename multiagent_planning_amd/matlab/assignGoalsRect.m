function [perm,pf,owner,cost,rounds] = assignGoalsRect(po,goals,prm,epsilon,max_rounds)
% Goal assignment with another number of goals than agents (no reference counterpart; assignGoals.m is the square case).
% po: 3 x N (or 1 x 3 x N as randomTest returns it), goals: 3 x M, max(N,M) <= 1024; prm: a dmpc_params_struct (its c sets the metric
% E1 = diag(1,1,1/c)).  Of all ways to match min(N,M) agent-goal pairs the one that minimises the sum of |E1 (po_i - goals_j)|^2 over the
% pairs, to within min(N,M)*epsilon (default 1e-4 / max(N,M)).
% perm (1 x N, 1-based): agent i flies to goals(:,perm(i)) = pf(:,i); perm(i) = 0: agent i has no goal and pf(:,i) = po(:,i), it stays.
% owner (1 x M, 1-based): goal j is taken by agent owner(j); 0: it stays empty.  cost: the sum over the pairs; rounds: auction rounds
% (-1: the cap max_rounds was met, perm and owner are then all zeros).
po = reshape(po,3,[]); goals = reshape(goals,3,[]);
if nargin < 4, epsilon = []; end
if nargin < 5, max_rounds = 0; end
[perm,pf,owner,cost,rounds] = dmpc_mex('assign_rect', prm, po, goals, epsilon, max_rounds);
end
